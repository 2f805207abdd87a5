"""The conv plan's routes held per channel, at unequal levels.  The FFT routes pack channels 2q and 2q + 1 into one
complex transform, so a channel's rounding error follows its PAIR's level (conv_pair_twin.py); the accuracy gates
elsewhere divide the largest error by one global peak, with every channel at the same level.  Here every route of
test_conv_plan_state_gpu.ROUTES that gab_conv_create / _create_scheme can pick is held, per channel, to

    c_t = max |y_t - truth_t| / (peak_t + peak_p)  <=  4 c_twin          (never above the suite's 1e-5)

where truth is the float64 whole-stream convolution (test_conv_fdl_host.stream_reference) and c_twin the same figure
of the float32 packed-pair restatement of that route's cut on the same input.  The factor 4 is the project's
precedent for a float32 form against its restatement (4 e32 for gab_iir's scan): room for radix-16 / radix-4 passes
and a folded 1/N that round differently from scipy's transform, none for a lost digit.  The direct route packs
nothing: its figure is over peak_t alone.

Every stream is fill_len + wrap_len + 4 buffers, run once per buffer and once through process_batch (on the split
route: conv_split_batch12_kernel), the two held to the same bits.  The engine and the round trip are held to these
launches bit for bit by test_gpu_parity.py."""
import numpy as np
import pytest

import conv_pair_twin as tw
from test_conv_fdl_host import stream_reference
from test_conv_plan_state_gpu import (ROUTES, dev, expected_state_bytes, fill_len, gab, host, make,  # noqa: F401
                                      same_bits)

pytestmark = pytest.mark.gpu

TOL = 1e-5              # the suite's gate against float64: no bound here is above it
FACTOR = 4.0
# The one case over the factor 4, gated at 1.5 x its measured ratio (4.500, profiles/r18_conv_levels.txt): the unit impulse
# on uniform-1024.  An impulse's spectrum is the bare product of the passes' twiddles, and the kernels form a pass's
# twiddle powers in registers from one table entry (gab_fft.hpp powers_of: up to four chained products, so up to four
# roundings per power) where scipy reads each from a table rounded once: on this input the restatement is nearly exact
# (c_twin 4.3e-8, a fifth of its figure on noise) while the kernel loses 1.9e-7 of the pair's level, less than on noise.
# Every other known answer on every route measures at most 4 (4.000 exactly three times on the uniform routes: the
# errors of these cases are whole numbers of ulps) and is gated at 4, as is every route on noise.
KNOWN_FACTOR = {("uniform-1024", "impulse"): 6.75}


@pytest.fixture(params=list(tw.LEVEL_ROUTES))
def route(request, gab):
    """Each case first proves the route it names: the scheme the plan reports and its state's size."""
    name = request.param
    T, B, L, arg, scheme, kind = ROUTES[name]
    p = gab.ConvPlan(T, B, L, scheme=arg)
    try:
        assert p.scheme == scheme
        assert tuple(p.state_bytes()) == expected_state_bytes(T, B, L, kind), name
    finally:
        p.close()
    return name


def shape(route):
    T, B, L, _, _, kind = ROUTES[route]
    return T, B, L, kind


def run_both(make, route, ir, xs, same=same_bits):
    """The stream through one launch per buffer and through process_batch: the same bits; returns the outputs."""
    n, size = len(xs), xs[0].size
    a, b = make(route, ir), make(route, ir)
    ys = [host(a.process(dev(x))) for x in xs]
    yb = host(b.process_batch(dev(np.concatenate(xs)), n)).reshape(n, size)
    for i in range(n):
        assert same(ys[i], yb[i]), (route, "batch differs at buffer", i)
    a.close()
    b.close()
    return ys


def bound(c_twin, factor=FACTOR):
    return min(factor * c_twin, TOL)


def same_bits_or_nan(a, b):
    """Bit for bit, but a NaN equals a NaN: its sign and payload are whatever the last instruction left."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


_cache = {}


def measured(make, route, what):
    """(ir, xs, truth, twin, gpu) of a route's unequal-levels ("levels") or silence stream: computed once."""
    key = (route, what)
    if key not in _cache:
        T, B, L, kind = shape(route)
        lv = tw.levels(T) if what == "levels" else SILENCE[:T]
        ir, xs = tw.levels_case(T, B, L, kind, lv, seed=1 if what == "levels" else 3)
        truth = stream_reference(xs, ir, T, B, L)
        twin = tw.twin_stream(kind, xs, ir, T, B, L)
        _cache[key] = (ir, xs, truth, twin, run_both(make, route, ir, xs))
    return _cache[key]


# (a) ----------------------------------------------------------------------------------------------------------------
def test_every_channel_is_within_4_c_twin_of_its_pairs_level(make, route):
    """Levels 1, 2^-10 | 1, 0 | 2^-20, 2^-20 | 1, 1 (cut to T): loud/quiet, loud/silent, quiet/quiet, loud/loud.  The
    quiet/quiet pair is divided by its own 2^-20 level: a pair's error follows the pair, not the plan."""
    T, B, L, kind = shape(route)
    ir, xs, truth, twin, ys = measured(make, route, "levels")
    first, paired = fill_len(B, L), kind in tw.PAIRED
    ct, level = tw.channel_figures(twin, truth, T, B, first, paired)
    cg, _ = tw.channel_figures(ys, truth, T, B, first, paired)
    c_twin = tw.c_max(ct)
    print("\n%s c_twin %.3g c_gpu %.3g ratio %.2f\n  twin %s\n  gpu  %s\n  level %s" % (
        route, c_twin, tw.c_max(cg), tw.c_max(cg) / c_twin, ct, cg, level))
    assert c_twin <= (2.5e-6 if kind == "direct" else 1e-6)          # the input's condition (the host tests)
    assert np.isfinite(cg).all()
    assert (cg <= bound(c_twin)).all(), (cg / c_twin)


# (b) ----------------------------------------------------------------------------------------------------------------
SILENCE = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0])         # loud/silent, a silent pair, loud/loud, a silent pair


def test_silence(make, route):
    """A silent pair gives zeros (either sign) beside loud pairs; on the direct route so does a silent channel beside
    a loud neighbour.  A silent channel packed with a loud partner gives the partner's rounding error, below
    4 c_twin of the partner's peak.  (uniform-1024 has two channels, one pair: it has no silent pair beside a loud one,
    and holds the loud/silent pair only; every other shape has a silent pair, which is asserted.)"""
    T, B, L, kind = shape(route)
    ir, xs, truth, twin, ys = measured(make, route, "silence")
    y, r = tw.per_channel(ys, T, B), tw.per_channel(truth, T, B)
    ct, level = tw.channel_figures(twin, truth, T, B, 0, kind in tw.PAIRED)
    c_twin = tw.c_max(ct)
    peaks = np.abs(r).max(axis=(1, 2))
    assert peaks[0] > 0 and not peaks[1:4].any()
    silent_pairs = [q for q in range((T + 1) // 2) if not peaks[2 * q:2 * q + 2].any()]
    assert silent_pairs or T < 3, route
    for t in range(T):
        partner = peaks[t ^ 1] if (t ^ 1) < T else 0.0
        if peaks[t] > 0:
            continue
        if kind == "direct" or partner == 0:
            assert not y[t].any(), (route, t)                        # y == 0, either sign
        else:
            got = np.abs(y[t]).max()
            print("\n%s silent channel %d: %.3g of the partner's peak (%.1f dB), twin %.3g" % (
                route, t, got / partner, 20 * np.log10(max(got / partner, 1e-300)), ct[t]))
            assert got <= bound(c_twin) * partner, (route, t, got / partner, c_twin)


def test_a_silent_channel_beside_a_loud_partner_is_not_silent(make, gab):
    """What include/gab_c_api.h says of the packed routes: the silent channel of a loud pair is NOT zeros."""
    T, B, L, kind = shape("classic-T6")
    ir, xs, truth, twin, ys = measured(make, "classic-T6", "silence")
    y = tw.per_channel(ys, T, B)
    assert y[1].any() and not y[2:4].any()


# (c) ----------------------------------------------------------------------------------------------------------------
def test_a_pair_is_a_function_of_its_own_pair(make, route):
    """Every pair in turn (pair 0, the last pair, and on the split route both pairs of each duo, whose transforms share
    a workgroup's LDS in the batch kernel): with every OTHER pair's input and response replaced by another seed at
    2^10 times the level, the watched pair's output is the same bits."""
    T, B, L, kind = shape(route)
    ir, xs, truth, twin, ys = measured(make, route, "levels")
    base = tw.per_channel(ys, T, B)
    ir2, xs2 = tw.levels_case(T, B, L, kind, np.full(T, 2.0 ** 10), seed=5)
    ir2 = ir2 * np.float32(2.0 ** 10)
    for q in range((T + 1) // 2):
        own = [t for t in (2 * q, 2 * q + 1) if t < T]
        irv = ir2.reshape(T, L).copy()
        irv[own] = ir.reshape(T, L)[own]
        xv = []
        for x, x2 in zip(xs, xs2):
            v = x2.reshape(T, B).copy()
            v[own] = x.reshape(T, B)[own]
            xv.append(v.ravel())
        got = tw.per_channel(run_both(make, route, irv.ravel(), xv), T, B)
        assert same_bits(got[own], base[own]), (route, "pair", q)
        others = [t for t in range(T) if t not in own]
        if others:
            assert not same_bits(got[others], base[others])


# (d) ----------------------------------------------------------------------------------------------------------------
def test_a_nan_and_an_infinity_stay_in_their_pairs_and_leave(make, route):
    """A NaN at one sample of channel 0 in buffer i (past the fill), an infinity in the last channel two buffers later,
    a clean twin stream beside it.  A pair that holds neither is the clean run's bits in every buffer.  A struck pair
    is non-finite, the struck channel's partner included, in every buffer whose taps reach the sample, and the clean
    run's bits again tw.nan_stay() buffers after the strike: when no window of the route holds the sample any more
    (exactly then on the packed routes, the split cut at most one buffer sooner; the direct form no later)."""
    T, B, L, kind = shape(route)
    stay = tw.nan_stay(kind, B, L)
    i = fill_len(B, L) + 1
    n = max(tw.stream_len(T, B, L, kind), i + 2 + stay + 2)
    ir = tw.decaying_ir(T, L, B, 7)
    xs = tw.noise(T, B, n, 8, tw.levels(T))
    strikes = [(0, i, B // 3, np.nan), (T - 1, i + 2, B - 1, np.inf)]
    xd = [x.copy() for x in xs]
    for t, k, s, v in strikes:
        xd[k][t * B + s] = v
    clean = tw.per_channel(run_both(make, route, ir, xs), T, B)
    # (the two launch forms of the split cut, and of no other route, leave NaNs of different sign in the struck pair)
    dirty = tw.per_channel(run_both(make, route, ir, xd, same_bits_or_nan if kind == "split" else same_bits), T, B)
    assert np.isfinite(clean).all()
    units = [[t] for t in range(T)] if kind == "direct" else [[t for t in (2 * q, 2 * q + 1) if t < T]
                                                              for q in range((T + 1) // 2)]
    stayed = {}
    for unit in units:
        hits = [h for h in strikes if h[0] in unit]
        first = min([h[1] for h in hits], default=n)
        again = max([h[1] + stay for h in hits], default=n)
        for k in range(n):
            if k < first or k >= again:
                assert same_bits(dirty[unit, k], clean[unit, k]), (route, unit, k)
        for t, k0, s, v in hits:
            for k in range(k0, min(n, (k0 * B + s + L - 1) // B + 1)):
                for u in unit:                                       # the struck channel and its partner
                    assert not np.isfinite(dirty[u, k]).all(), (route, u, k)
        if hits:
            differs = [k for k in range(n) if not same_bits(dirty[unit, k], clean[unit, k])]
            stayed[tuple(unit)] = (first, differs[-1] - first + 1)
            # the figure is the count itself where a transform holds the sample; the split cut's far share comes a
            # buffer ahead for a pair every other buffer (one buffer less at one parity of the strike), and the direct
            # form's count depends on where in its buffer the sample lies
            if kind == "split":
                assert again - first - 1 <= stayed[tuple(unit)][1] <= again - first, (route, unit, stayed)
            elif kind != "direct":
                assert stayed[tuple(unit)][1] == again - first, (route, unit, stayed)
    print("\n%s nan_stay %d; struck units (first buffer, buffers until the clean bits): %s" % (route, stay, stayed))


# (e) ----------------------------------------------------------------------------------------------------------------
def test_one_hot_taps_at_partition_edges_delay_the_input(make, route):
    """One tap per channel at the route's partition edges (512-sample cuts: 0, 511, 512, 1023, 1024, 2047, 2048, 4095):
    the output is the input delayed by that many samples, within 4 c_twin of the pair's level."""
    T, B, L, kind = shape(route)
    xs = tw.noise(T, B, tw.stream_len(T, B, L, kind), 9)
    paired = kind in tw.PAIRED
    worst = 0.0
    for taps, ir in tw.one_hot_cases(T, B, L, kind):
        want = tw.delayed(xs, taps, T, B)
        ct, _ = tw.channel_figures(tw.twin_stream(kind, xs, ir, T, B, L), want, T, B, 0, paired)
        cg, _ = tw.channel_figures(run_both(make, route, ir, xs), want, T, B, 0, paired)
        c_twin = tw.c_max(ct)
        if c_twin > 0:
            worst = max(worst, tw.c_max(cg) / c_twin)
        print("\n%s taps %s c_twin %.3g c_gpu %.3g" % (route, taps, c_twin, tw.c_max(cg)))
        assert c_twin <= 1e-6
        assert (cg <= bound(c_twin, KNOWN_FACTOR.get((route, "one-hot"), FACTOR))).all(), (taps, cg, c_twin)
    print("%s worst ratio %.3f" % (route, worst))


def test_a_unit_impulse_gives_the_response(make, route):
    """A unit impulse on every channel at the first sample of the stream: the output is the response itself, buffer
    by buffer (and zeros to rounding after its end), within 4 c_twin of the pair's level (uniform-1024: KNOWN_FACTOR)."""
    T, B, L, kind = shape(route)
    n = tw.stream_len(T, B, L, kind)
    ir = tw.decaying_ir(T, L, B, 10)
    xs = [np.zeros(T * B, np.float32) for _ in range(n)]
    xs[0].reshape(T, B)[:, 0] = 1.0
    want = np.zeros((T, n * B))
    want[:, :L] = ir.reshape(T, L)
    want = [np.ascontiguousarray(want[:, k * B:(k + 1) * B].T).ravel() for k in range(n)]
    paired = kind in tw.PAIRED
    ct, _ = tw.channel_figures(tw.twin_stream(kind, xs, ir, T, B, L), want, T, B, 0, paired)
    cg, _ = tw.channel_figures(run_both(make, route, ir, xs), want, T, B, 0, paired)
    c_twin = tw.c_max(ct)
    print("\n%s impulse c_twin %.3g c_gpu %.3g ratio %.3f" % (route, c_twin, tw.c_max(cg), tw.c_max(cg) / max(c_twin, 1e-300)))
    assert c_twin <= 1e-6
    assert (cg <= bound(c_twin, KNOWN_FACTOR.get((route, "impulse"), FACTOR))).all(), (cg, c_twin)
