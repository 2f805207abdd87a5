"""The limiter plan (gab_lim_*) on the device.

Every comparison is on bit patterns against tests/limiter_twin.py (held by tests/test_limiter_host.py): outputs, the
gain-reduction meter and the three histories.  The contract fixes every rounding, so the kernel has no freedom.  The
reference streams are computed once per (shape, scenario) and shared, read only.

The kernel's cut (k_limiter.hip): a wave owns 8 tracks and walks chunks of 64 samples with a lane per sample; a link
group of up to 8 tracks is reduced inside the wave's registers, one of 16, 32 or 64 by a launch in front; the rings hold
max(W, 64) samples of history, so k <= 6, k = 7 and k = 8 are three shapes of the window recursion; 16-byte aligned blocks
with bufsize % 4 == 0 take the wide load.  The shapes below cross every one of those edges.
"""
import ctypes
import functools

import numpy as np
import pytest

from limiter_twin import CEIL, FIELDS, IDENTITY, REL, Twin, levels, lim_mix, table
from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_mix_host import Twin as MixTwin
from test_mix_host import gains as mix_gains

pytestmark = pytest.mark.gpu

# (tracks, bufsize, k, link): every value of tracks {1, 3, 64, 65, 130}, bufsize {1, 5, 63, 64, 65, 200, 512}, k {2, 5, 6,
# 8} and link {1, 2, 64}; buffers shorter than W - 1 (5 and 1 against 31 and 255), a short last wave (65, 130, 3), one
# sample, link groups inside the wave and wider than it, and the two at that edge (8 and 16); k = 7, the ring of two
# history passes, in single words (bufsize 70), in 16-byte loads (200), shorter than W - 1 (5) and behind the launch in
# front (link 32)
SHAPES = [(65, 70, 7, 1), (40, 200, 7, 2), (9, 5, 7, 1), (64, 72, 7, 32), (24, 70, 6, 8), (48, 64, 5, 16), (1, 1, 2, 1), (3, 5, 5, 1), (64, 63, 6, 64), (65, 64, 8, 1), (130, 65, 2, 2), (64, 200, 8, 64), (130, 512, 5, 2),
          (3, 200, 6, 1), (65, 5, 8, 1), (1, 64, 5, 1), (130, 1, 8, 2), (64, 65, 5, 64), (64, 512, 6, 2)]
N = 6
SMALL = (70, 100, 5, 2)            # the shape of the single scenarios; WIDE: the same through the launch in front, W = 256
WIDE = (128, 72, 8, 64)
MID = (70, 100, 7, 2)              # and W = 128


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def run(plan, x, with_gr=True, out=None):
    """x [T][B] numpy -> (y [T][B], gr [T] or None) numpy"""
    import torch
    gr = torch.full((plan.tracks,), 7.0, device="cuda") if with_gr else None
    y = plan.process(dev(x.ravel()), gr=gr)
    return host(y).reshape(plan.tracks, plan.bufsize), (host(gr) if with_gr else None)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def same_state(plan, twin):
    return all(same(host(a), b) for a, b in zip(plan.state(), twin.hist))


def make(gab, T, B, k, link, p=None):
    plan = gab.LimiterPlan(T, B, 1 << k, link)
    assert (plan.tracks, plan.bufsize, plan.lookahead, plan.link, plan.latency) == (T, B, 1 << k, link, (1 << k) - 1)
    if p is not None:
        plan.set_params(dev(p), ramp=False)
    return plan


@functools.lru_cache(maxsize=None)
def stream(T, B, k, link, ramp_at=None, n=N):
    """The shared scenario: lim_mix(seed 1) at once, lim_mix(seed 2) set with a ramp before buffer ramp_at, n buffers of
    noise at a level per track.  Returns (p0, p1, xs [n][T][B], ys, grs [n][T], the histories after each buffer, the
    twin afterwards); read only."""
    p0, p1 = lim_mix(T, 1), lim_mix(T, 2)
    twin = Twin(T, B, 1 << k, link)
    twin.set_params(p0, ramp=False)
    xs = np.stack([levels(T, B, 1000 + i) for i in range(n)])
    ys, grs, hists = [], [], []
    for i in range(n):
        if i == ramp_at:
            twin.set_params(p1)
        y, gr = twin.process(xs[i])
        ys.append(y), grs.append(gr), hists.append(twin.hist)
    ys, grs = np.stack(ys), np.stack(grs)
    for a in (p0, p1, xs, ys, grs):
        a.setflags(write=False)
    return p0, p1, xs, ys, grs, hists, twin


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,k,link", SHAPES)
def test_contract_bit_for_bit(gab, T, B, k, link):
    """Six buffers at a table that limits on some tracks and not on others; the outputs, the meter and, at the end, the
    three histories."""
    p0, _, xs, ys, grs, hists, twin = stream(T, B, k, link)
    plan = make(gab, T, B, k, link, p0)
    for i in range(N):
        y, gr = run(plan, xs[i], with_gr=i != 2)
        assert same(y, ys[i]), i
        assert gr is None or same(gr, grs[i]), i
    assert same_state(plan, twin)
    assert T * B * N < 300 or T == 1 or (grs < 1.0).any()             # the scenario limits
    assert T < 64 or B < 64 or link == 64 or (grs == 1.0).any()       # and, unless all share a detector, on some tracks it does not
    plan.close()


def test_a_new_plan_is_a_pure_delay(gab):
    for T, B, k, link in ((7, 50, 4, 1), (128, 64, 8, 64)):
        plan, D = make(gab, T, B, k, link), (1 << k) - 1
        ident = np.tile(IDENTITY, (T, 1))
        assert same_params(plan, ident, ident)
        x = (np.random.RandomState(5).uniform(-1.0, 1.0, (T, 6 * B)) * 2.0 ** 31).astype(np.float32)
        x[0, 3], x[T - 1, B - 1], x[T // 2, 0] = np.inf, np.nan, -0.0
        got = np.concatenate([run(plan, x[:, i * B:(i + 1) * B])[0] for i in range(6)], axis=1)
        assert same(got, np.concatenate([np.zeros((T, D), np.float32), x[:, :6 * B - D]], axis=1))
        plan.close()


def test_buffers_shorter_than_the_window(gab):
    """bufsize 3 and 40 against W - 1 = 63 and 255: the histories move by less than their length per call."""
    for T, B, k, link in ((20, 3, 6, 4), (33, 40, 8, 1)):
        p0, _, xs, ys, grs, hists, twin = stream(T, B, k, link, None, 12)
        plan = make(gab, T, B, k, link, p0)
        for i in range(12):
            y, gr = run(plan, xs[i])
            assert same(y, ys[i]) and same(gr, grs[i]), i
            if i in (0, 5, 11):
                assert all(same(host(a), b) for a, b in zip(plan.state(), hists[i])), i
        assert (grs[-1] < 1.0).any()
        plan.close()


# ---- 2. batches, ramps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, WIDE, MID])
@pytest.mark.parametrize("n", [1, N])
def test_batch_is_n_single_launches(gab, shape, n):
    """A ramp is pending in front of the batch.  The batch, n per-buffer calls and the reference agree; so do the two
    plans' histories and tables afterwards."""
    import torch
    T, B, k, link = shape
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0)
    a, b = make(gab, T, B, k, link, p0), make(gab, T, B, k, link, p0)
    for p in (a, b):
        p.set_params(dev(p1))
        assert same_params(p, p0, p1)
    singles = [run(a, xs[i]) for i in range(n)]
    gr = torch.full((n * T,), 7.0, device="cuda")
    batch = host(b.process_batch(dev(xs[:n].ravel()), gr=gr)).reshape(n, T, B)
    assert same(batch, np.stack([s[0] for s in singles])) and same(batch, ys[:n])
    assert same(host(gr).reshape(n, T), np.stack([s[1] for s in singles])) and same(host(gr).reshape(n, T), grs[:n])
    for p in (a, b):
        assert all(same(host(u), v) for u, v in zip(p.state(), hists[n - 1]))
        assert same_params(p, p1, p1)
    if n < N:                                                         # and the stream goes on
        assert same(run(b, xs[n])[0], ys[n])
    a.close()
    b.close()


def test_a_ramp_mid_stream_and_mixed_calls(gab):
    T, B, k, link = SMALL
    p0, p1, xs, ys, grs, hists, twin = stream(T, B, k, link, 2)
    plan = make(gab, T, B, k, link, p0)
    got = [run(plan, xs[0], with_gr=False)[0][None], host(plan.process_batch(dev(xs[1:2].ravel()))).reshape(1, T, B)]
    plan.set_params(dev(p1))                                          # the ramp runs through the batch's first buffer
    got.append(host(plan.process_batch(dev(xs[2:5].ravel()))).reshape(3, T, B))
    got.append(run(plan, xs[5], with_gr=False)[0][None])
    assert same(np.concatenate(got), ys) and same_state(plan, twin) and same_params(plan, p1, p1)
    assert (bits(ys[2]) != bits(stream(T, B, k, link)[3][2])).any()    # the ramp changed the bits
    plan.close()


# ---- 3. in place, unaligned -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, WIDE, MID, (130, 512, 5, 2)])
def test_in_place_and_unaligned(gab, shape):
    import torch
    T, B, k, link = shape
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0 if shape != (130, 512, 5, 2) else None)
    a, b, c = (make(gab, T, B, k, link, p0) for _ in range(3))
    for i in range(2):
        if i == 0 and shape != (130, 512, 5, 2):
            for p in (a, b, c):
                p.set_params(dev(p1))
        buf = dev(xs[i].ravel())
        assert a.process(buf, out=buf) is buf                                    # in place
        assert same(host(buf).reshape(T, B), ys[i]), i
        big = torch.zeros(T * B + 1, device="cuda")
        big[1:] = dev(xs[i].ravel())
        out = torch.full((T * B + 3,), 7.0, device="cuda")
        b.process(big[1:], out=out[1:T * B + 1])                                 # in and out 4 bytes off alignment
        o = host(out)
        assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all()
        assert same(o[1:T * B + 1].reshape(T, B), ys[i]), i
        c.process(big[1:], out=big[1:])                                          # in place and unaligned
        assert same(host(big)[1:].reshape(T, B), ys[i]), i
    for p in (a, b, c):
        assert all(same(host(u), v) for u, v in zip(p.state(), hists[1]))
        p.close()


# ---- 4. parameters moved mid-stream -----------------------------------------------------------------------------
def test_set_params_mid_stream(gab):
    """Ramp 1 and 0, two sets before one buffer, a middle range of tracks, a reset in the stream."""
    T, B, k, link = SMALL
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0)
    p2 = lim_mix(T, 3)
    plan, twin, still = make(gab, T, B, k, link, p0), Twin(T, B, 1 << k, link), make(gab, T, B, k, link, p0)
    twin.set_params(p0, ramp=False)
    moved = np.zeros(T, bool)
    moved[20:40] = True
    for i in range(N):
        if i == 1:                                                    # two sets before a buffer: the ramp starts from current
            for q in (p2[20:40], p1[20:40]):
                plan.set_params(dev(q), first_track=20)
                twin.set_params(q, first_track=20)
        if i == 3:
            plan.set_params(dev(p2[30:40]), ramp=False, first_track=30)         # at once
            twin.set_params(p2[30:40], ramp=False, first_track=30)
        if i == 4:
            plan.set_params(dev(p0[20:40]), first_track=20)
            twin.set_params(p0[20:40], first_track=20)
            plan.reset()                                              # drops that ramp, keeps its target, clears the histories
            twin.reset()
            still.reset()
            hx, ht, he = (host(a) for a in plan.state())
            assert not hx.any() and (ht == 1.0).all() and (he == 1.0).all()
        assert same_params(plan, twin.cur, twin.tgt), i
        (y, gr), (ys_still, _) = run(plan, xs[i]), run(still, xs[i])
        want, want_gr = twin.process(xs[i])
        assert same(y, want) and same(gr, want_gr), i
        assert same(y[~moved], ys_still[~moved]), i                   # no other track's bits change
        assert same_params(plan, twin.cur, twin.tgt) and same_state(plan, twin), i
        if i in (1, 3):
            assert (bits(y[moved]) != bits(ys_still[moved])).any()
    plan.close()
    still.close()


# ---- 5. a shard -------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, B, k, link = SMALL
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0)
    lo, hi = 6, 70                                                    # a multiple of link that is no multiple of 16
    shard = make(gab, hi - lo, B, k, link, p0[lo:hi])
    shard.set_params(dev(p1[lo:hi]))
    for i in range(3):
        y, gr = run(shard, xs[i, lo:hi])
        assert same(y, ys[i, lo:hi]) and same(gr, grs[i, lo:hi]), i
    assert all(same(host(u), v[lo:hi]) for u, v in zip(shard.state(), hists[2]))
    shard.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    T, B, k, link = SMALL
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 1)
    plan = make(gab, T, B, k, link, p0)
    assert same(run(plan, xs[0])[0], ys[0])
    plan.set_params(dev(p1))
    before = [host(a) for a in plan.state()]
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))     # noqa: E731
    down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    cases = [(np.nan, (4, 0)), (np.inf, (0, 0)), (np.float32(-1e-30), (9, 0)), (up(2.0 ** 32), (3, 0)),
             (np.nan, (69, 1)), (0.0, (5, 1)), (down(2.0 ** -32), (6, 1)), (up(2.0 ** 32), (7, 1)), (-np.inf, (8, 1)),
             (np.nan, (10, 2)), (np.float32(-1e-30), (11, 2)), (up(1.0), (12, 2)), (np.inf, (13, 2))]
    assert {w[1] for _, w in cases} == set(range(FIELDS))              # every field
    for value, where in cases:
        bad = lim_mix(T, 3)
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, 0] = np.nan                             # the FIRST offender is named
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d" % where in str(e.value), str(e.value)
    bad = lim_mix(4, 3)
    bad[2, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), first_track=3)
    assert "track 5 field 1" in str(e.value)
    edge = make(gab, 3, B, k, 1)                                      # the edges themselves are admitted
    edge.set_params(dev(np.array([[0.0, 2.0 ** -32, 0.0], [2.0 ** 32, 2.0 ** 32, 1.0], [-0.0, 1.0, -0.0]], np.float32)))
    edge.close()
    assert same_params(plan, p0, p1) and all(same(host(a), b) for a, b in zip(plan.state(), before))
    for i in (1, 2):                                                  # the pending ramp is still pending
        assert same(run(plan, xs[i])[0], ys[i]), i
    plan.close()


def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, k, link = SMALL
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 6, 1), (4, 0, 6, 1), (4, 64, 1, 1), (4, 64, 9, 1), (4, 64, 6, 3), (4, 64, 6, 128), (6, 64, 6, 4)):
        assert lib.gab_lim_create(ctypes.byref(h), *args) == bad and not h.value, args
    with pytest.raises(gab.GabError):
        gab.LimiterPlan(5, 64, 64, 2)
    for lookahead in (0, 3, 48, 2, 512):
        with pytest.raises((ValueError, gab.GabError)):
            gab.LimiterPlan(4, 64, lookahead)
    plan = make(gab, T, B, k, link, p0)
    plan.set_params(dev(p1))
    hp = plan._h
    import torch
    big = torch.zeros(2 * T * B + 8, device="cuda")
    big[:T * B] = dev(xs[0].ravel())
    out, pd = dev(np.zeros(T * B, np.float32)), dev(p0)
    at = lambda off: ctypes.c_void_p(big.data_ptr() + 4 * off)         # noqa: E731
    q, o, pp = at(0), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(pd.data_ptr())
    assert lib.gab_lim_process(hp, None, o, None, None) == bad and lib.gab_lim_process(hp, q, None, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    for off in (1, 4, T * B - 1, T * B // 2):                    # every overlap but d_out == d_in
        assert lib.gab_lim_process(hp, q, at(off), None, None) == bad and b"overlap" in lib.gab_last_error(), off
    assert lib.gab_lim_process(hp, at(4), q, None, None) == bad
    assert lib.gab_lim_process_batch(hp, q, at(T * B), None, 2, None) == bad and b"overlap" in lib.gab_last_error()
    assert lib.gab_lim_process_batch(hp, q, o, None, 0, None) == bad and lib.gab_lim_process_batch(hp, q, o, None, -3, None) == bad
    assert lib.gab_lim_set_params(hp, None, 1, None) == bad and lib.gab_lim_set_params(None, pp, 1, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_lim_set_params_tracks(hp, pp, first, n, 1, None) == bad, (first, n)
    assert lib.gab_lim_params(hp, None, None, None) == bad and lib.gab_lim_state(hp, None, None, None, None) == bad
    assert lib.gab_lim_latency(hp, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:7]))
    with pytest.raises(ValueError):
        plan.set_params(dev(p0[:3]))
    for i in range(2):                                                # nothing above touched the plan
        assert same(run(plan, xs[i])[0], ys[i]), i
    plan.close()


# ---- 7. the guarantee, the subnormals, samples that are not finite ------------------------------------------------
def test_the_ceiling_holds_on_the_devices_own_output(gab):
    T, B, n = 40, 256, 4
    for k, link in ((3, 1), (6, 2), (8, 1)):
        rels = np.array((0.0, 0.01, 0.3, 1.0), np.float32)
        p = table(T)
        p[:, CEIL] = np.array((1.0, 0.891, 0.999999, 1.2345, 0.5), np.float32)[np.arange(T) % 5]
        p[:, REL] = rels[(np.arange(T) // 5) % 4]
        x = (np.random.RandomState(k).uniform(-1.0, 1.0, (n, T, B)) * 50.0 * p[None, :, CEIL:CEIL + 1]).astype(np.float32)
        plan = make(gab, T, B, k, link, p)
        y = host(plan.process_batch(dev(x.ravel()))).reshape(n, T, B)
        assert (np.abs(y) <= p[None, :, CEIL:CEIL + 1]).all()          # <=, no tolerance
        assert (np.abs(y[1:]) > 0.5 * p[None, :, CEIL:CEIL + 1]).any()
        plan.close()


def test_a_tail_through_the_subnormals(gab):
    """ceil = 2^-32 against samples near FLT_MAX: the need is subnormal or zero, the box sums subnormals, and the bits
    still agree; the output stays at or below 2^-32."""
    T, B, k = 18, 96, 4
    p = table(T, ceil=2.0 ** -32, rel=0.25)
    p[1::2, REL] = 0.0
    rng = np.random.RandomState(3)
    xs = (rng.uniform(-1.0, 1.0, (4, T, B)) * np.exp2(rng.uniform(80.0, 127.9, (4, T, B)))).astype(np.float32)
    xs[2:] *= np.float32(2.0 ** -120)                                  # and back up out of the subnormals
    plan, twin = make(gab, T, B, k, 1, p), Twin(T, B, 1 << k, 1)
    twin.set_params(p, ramp=False)
    tiny = False
    for i in range(4):
        y, gr = run(plan, xs[i])
        want, want_gr = twin.process(xs[i])
        assert same(y, want) and same(gr, want_gr) and same_state(plan, twin), i
        assert (np.abs(y) <= np.float32(2.0 ** -32)).all()
        tiny = tiny or bool(((twin.g < 2.0 ** -126) & (twin.g > 0)).any() and (twin.g == 0).any())
    assert tiny                                                       # the scenario reaches subnormal and zero gains
    plan.close()


@pytest.mark.parametrize("shape", [(66, 100, 5, 2), WIDE])
def test_nonfinite_samples_reach_one_output_sample_and_nothing_else(gab, shape):
    T, B, k, link = shape
    D = (1 << k) - 1
    p = lim_mix(T, 1)
    plans, twin = [make(gab, T, B, k, link, p) for _ in range(2)], Twin(T, B, 1 << k, link)
    twin.set_params(p, ramp=False)
    n = 2 + (D + B - 1) // B
    spots = [(0, 0, 10), (0, 1, 50), (1, T - 1, B - 1), (1, 30, 0)]    # (buffer, track, sample)
    outs = []
    for i in range(n):
        x = levels(T, B, 60 + i)
        x0 = x.copy()
        for v, (b, t, s) in zip((np.nan, np.inf, -np.inf, np.nan), spots):
            if b == i:
                x[t, s], x0[t, s] = v, 0.0
        (y, gr), (y0, gr0) = run(plans[0], x), run(plans[1], x0)
        want, want_gr = twin.process(x)
        assert same(y, want) and same(gr, want_gr) and same(gr, gr0) and same_state(plans[0], twin), i
        assert np.isfinite(gr).all()
        outs.append((y, y0))
        hx, ht, he = (host(a) for a in plans[0].state())
        hx0, ht0, he0 = (host(a) for a in plans[1].state())
        assert same(ht, ht0) and same(he, he0) and np.isfinite(ht).all() and np.isfinite(he).all(), i
    y, y0 = (np.concatenate([o[j] for o in outs], axis=1) for j in range(2))
    differ = bits(y) != bits(y0)
    assert differ.sum() == len(spots)
    for b, t, s in spots:
        assert differ[t, b * B + s + D] and not np.isfinite(y[t, b * B + s + D])
    assert same(hx, hx0)                                              # the slots have left the history
    for pl in plans:
        pl.close()


# ---- 8. a captured graph ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, WIDE, MID])
def test_graph_replay_gives_the_bits_of_plain_calls(gab, shape):
    import torch
    T, B, k, link = shape
    p0, p1, xs, ys, grs, hists, _ = stream(T, B, k, link, 0)
    plan = make(gab, T, B, k, link, p0)
    plan.set_params(dev(p1))
    assert same(run(plan, xs[0])[0], ys[0])                           # the ramp buffer, by a plain call
    x, out, gr = torch.zeros(T * B, device="cuda"), torch.zeros(T * B, device="cuda"), torch.zeros(T, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out, gr=gr)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the capture recorded a launch without running it: the histories are still those behind buffer 0
    assert all(same(host(u), v) for u, v in zip(plan.state(), hists[0]))
    for i in range(1, 4):
        x.copy_(dev(xs[i].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(T, B), ys[i]) and same(host(gr), grs[i]), i
    assert all(same(host(u), v) for u, v in zip(plan.state(), hists[3]))
    del graph
    plan.close()


# ---- 9. a strip --------------------------------------------------------------------------------------------------
def test_a_mix_bus_with_the_limiter_behind_it(gab):
    """MixPlan (48 tracks to 2 buses) into LimiterPlan (2 tracks, linked), in place on the bus block, against the two
    restatements composed."""
    T, M, B, k = 48, 2, 160, 6
    mix, lim = gab.MixPlan(T, B, M), make(gab, M, B, k, 2, table(M, drive=1.5, ceil=0.7, rel=0.002))
    mtwin, ltwin = MixTwin(T, B, M, *mix.form), Twin(M, B, 1 << k, 2)
    ltwin.set_params(table(M, drive=1.5, ceil=0.7, rel=0.002), ramp=False)
    g = mix_gains(T, M, 4)
    mix.set_gains(dev(g), ramp=False)
    mtwin.set_gains(g, ramp=False)
    hit = False
    for i in range(4):
        x = levels(T, B, 300 + i)
        if i == 2:
            g2 = mix_gains(T, M, 5)
            mix.set_gains(dev(g2))                                    # a fader move, ramped, under the limiter
            mtwin.set_gains(g2)
        bus = mix.process(dev(x.ravel()))
        assert lim.process(bus, out=bus) is bus
        want, gr = ltwin.process(mtwin.process(x))
        assert same(host(bus).reshape(M, B), want), i
        assert (np.abs(host(bus)) <= np.float32(0.7)).all()
        hit = hit or bool((gr < 1.0).any())
    assert hit and same_state(lim, ltwin)
    mix.close()
    lim.close()


def test_the_plan_releases_its_device_memory(gab):
    """Free device memory is back where it started after many create / use / close cycles."""
    import torch
    T, B = 16384, 128                                                 # 50 MiB of histories per plan at W = 256
    x = dev(levels(1, T * B, 9).ravel())
    out = torch.empty_like(x)
    p = dev(table(T, ceil=0.5, rel=0.01))

    def cycle():
        plan = gab.LimiterPlan(T, B, 256, 64)
        plan.set_params(p)
        plan.process(x, out=out)
        plan.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(10):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (64 << 20), (free0, free1)                 # 10 leaked plans would hold 500 MiB
