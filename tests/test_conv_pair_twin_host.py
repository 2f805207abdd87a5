"""Pins the float32 packed-pair yardstick (conv_pair_twin.py) without a GPU, so that the per-channel gates of
test_conv_levels_gpu.py and test_fft_levels_gpu.py rest on something checked: its accuracy against float64 on the
gates' own inputs, the figures of a silent and of a quiet channel beside a loud partner, exact scaling by powers of
two, and known answers at the partition edges."""
import numpy as np
import pytest

import conv_pair_twin as tw
from test_conv_fdl_host import stream_reference
from test_conv_plan_state_gpu import ROUTES, fill_len


def shape(route):
    T, B, L, _, _, kind = ROUTES[route]
    return T, B, L, kind


@pytest.mark.parametrize("route", tw.LEVEL_ROUTES)
def test_cut_covers_every_tap_once(route):
    T, B, L, kind = shape(route)
    cut = tw.route_cut(kind, B, L)
    if cut is None:
        assert kind == "direct"
        return
    assert cut[0][0] == 0 and cut[-1][1] == L
    assert all(a[1] == b[0] for a, b in zip(cut, cut[1:]))
    assert all(0 < e - f <= N - B + 1 for f, e, N in cut)


@pytest.mark.parametrize("route", tw.LEVEL_ROUTES)
def test_yardstick_is_within_1e6_of_float64_on_the_gates_inputs(route):
    """A condition on the inputs, not a tolerance for a kernel: a cut whose yardstick loses more than 1e-6 of the
    pair's level on the unequal-levels stream would make 4 c_twin a loose gate.  Measured: 2.0e-7 .. 2.4e-7 on every
    packed cut (the loud channels; their quiet or silent partners 0.9e-7 .. 1.3e-7).

    The direct form is no cut: it packs nothing and adds 700 products into one float32 accumulator, which loses
    0.9e-6 .. 1.3e-6 of the channel's own peak whatever the input (about sqrt(L) half-ulps).  Its restatement is held
    to 2.5e-6, so that 4 c_twin stays under the suite's 1e-5 there too."""
    T, B, L, kind = shape(route)
    ir, xs = tw.levels_case(T, B, L, kind)
    truth = stream_reference(xs, ir, T, B, L)
    ys = tw.twin_stream(kind, xs, ir, T, B, L)
    assert all(y.dtype == np.float32 for y in ys)
    c, level = tw.channel_figures(ys, truth, T, B, fill_len(B, L), kind in tw.PAIRED)
    print(route, "c_twin %.3g" % tw.c_max(c), c)
    assert tw.c_max(c) <= (2.5e-6 if kind == "direct" else 1e-6)
    if kind in tw.PAIRED:
        assert np.isfinite(c).all()                                # no pair of the levels is silent
        assert np.nanmin(c) >= 1e-8                                # the silent channel is not silent


def reverb_ir(T, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, L)) * np.exp(-np.arange(L) / (L / 5.0))).astype(np.float32).ravel()


def pair_errors(level_b, seed):
    """(error of A, error of B, peak of A, peak of B) of the classic cut: 512/4096 taps, 12 buffers, one pair."""
    T, B, L, n = 2, 512, 4096, 12
    ir = reverb_ir(T, L, seed)
    xs = tw.noise(T, B, n, seed + 10, [1.0, level_b])
    truth = tw.per_channel(stream_reference(xs, ir, T, B, L), T, B)
    y = tw.per_channel(tw.pair_stream(xs, ir, T, B, L, tw.route_cut("classic", B, L)), T, B).astype(np.float64)
    e, pk = np.abs(y - truth).max(axis=(1, 2)), np.abs(truth).max(axis=(1, 2))
    return e[0], e[1], pk[0], pk[1]


def within2(x, ref):
    return ref / 2 <= x <= ref * 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_channels_error_follows_its_partners_level(seed):
    """The table of the pair contract (include/gab_c_api.h, "channel pairs"), within a factor of 2:
        pair              err A / peak A   err B / peak A   err B / peak B
        equal levels      2.6e-7           2.6e-7           2.2e-7
        B at 2^-20 of A   1.9e-7           1.6e-7           0.14
        B silent          1.8e-7           1.1e-7           -"""
    ea, eb, pa, pb = pair_errors(1.0, seed)
    assert within2(ea / pa, 2.6e-7) and within2(eb / pa, 2.6e-7) and within2(eb / pb, 2.2e-7)
    ea, eb, pa, pb = pair_errors(2.0 ** -20, seed)
    assert within2(ea / pa, 1.9e-7) and within2(eb / pa, 1.6e-7) and within2(eb / pb, 0.14)
    assert eb / pb > 1e-2
    ea, eb, pa, pb = pair_errors(0.0, seed)
    assert pb == 0.0
    assert within2(ea / pa, 1.8e-7) and within2(eb / pa, 1.1e-7)
    assert 1e-8 <= eb / pa <= 1e-6


def test_a_silent_pair_gives_zeros():
    T, B, L, n = 4, 512, 4096, 10
    ir = reverb_ir(T, L, 4)
    xs = tw.noise(T, B, n, 5, [1.0, 1.0, 0.0, 0.0])
    y = tw.per_channel(tw.pair_stream(xs, ir, T, B, L, tw.route_cut("split", B, L)), T, B)
    assert not y[2:].any() and y[:2].any()


@pytest.mark.parametrize("route", ["split", "classic-T6", "uniform-256", "fdl-groups"])
@pytest.mark.parametrize("k", [-7, 5])
def test_scaling_a_pair_by_a_power_of_two_scales_its_output_exactly(route, k):
    T, B, L, kind = shape(route)
    ir = tw.decaying_ir(T, L, B, 6)
    xs = tw.noise(T, B, fill_len(B, L) + 3, 7, tw.levels(T))
    cut = tw.route_cut(kind, B, L)
    y = tw.pair_stream(xs, ir, T, B, L, cut)
    ys = tw.pair_stream([x * np.float32(2.0 ** k) for x in xs], ir, T, B, L, cut)
    for a, b in zip(y, ys):
        assert np.array_equal(a * np.float32(2.0 ** k), b)


@pytest.mark.parametrize("route", tw.LEVEL_ROUTES)
def test_one_hot_taps_at_partition_edges_delay_the_input(route):
    T, B, L, kind = shape(route)
    xs = tw.noise(T, B, fill_len(B, L) + 3, 8)
    seen = set()
    for taps, ir in tw.one_hot_cases(T, B, L, kind):
        seen |= set(taps)
        want = tw.delayed(xs, taps, T, B)
        c, _ = tw.channel_figures(tw.twin_stream(kind, xs, ir, T, B, L), want, T, B, 0, kind in tw.PAIRED)
        assert tw.c_max(c) <= (0.0 if kind == "direct" else 1e-6), (taps, c)
    assert seen == set(tw.edge_taps(kind, B, L)) and {0, L - 1} <= seen
    if kind in ("classic", "bank", "split"):
        assert sorted(seen) == list(tw.EDGES_512)


def test_delayed_is_the_float64_reference_of_a_one_hot_response():
    T, B, L = 3, 128, 1000
    xs = tw.noise(T, B, 12, 9)
    taps, ir = tw.one_hot_cases(T, B, L, "fdl")[1]
    for a, b in zip(tw.delayed(xs, taps, T, B), stream_reference(xs, ir, T, B, L)):
        assert np.abs(a - b).max() <= 1e-12


@pytest.mark.parametrize("kind,B,L,stay", [("fused", 512, 512, 2), ("classic", 512, 4096, 9), ("split", 512, 4096, 10),
                                           ("uniform", 256, 3000, 17), ("uniform", 1024, 16384, 17),
                                           ("uniform", 32, 700, 129), ("direct", 300, 700, 4), ("fdl", 512, 20000, 41),
                                           ("fdl", 128, 5000, 41)])
def test_nan_stay_figures_of_the_header(kind, B, L, stay):
    assert tw.nan_stay(kind, B, L) == stay


@pytest.mark.parametrize("kind,B,L", [("fused", 512, 512), ("classic", 512, 4096), ("split", 512, 4096),
                                      ("uniform", 256, 3000), ("fdl", 128, 1000)])
def test_a_nan_leaves_the_yardstick_no_later_than_nan_stay(kind, B, L):
    """A NaN leaves the yardstick when its last window does.  (The split cut's far window is eight blocks for seven
    blocks of taps, here as in the kernel: ten buffers, one more than the classic cut.)"""
    T, i = 2, 3
    stay = tw.nan_stay(kind, B, L)
    xs = tw.noise(T, B, i + stay + 2, 10)
    xs[i][B // 3] = np.nan
    y = tw.per_channel(tw.twin_stream(kind, xs, tw.decaying_ir(T, L, B, 11), T, B, L), T, B)
    bad = ~np.isfinite(y).all(axis=2)
    assert bad[:, i:i + stay].all() and not bad[:, :i].any() and not bad[:, i + stay:].any()


# ---- the 1024-point r2c ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 9, 17])
def test_fft_twin_is_within_1e6_of_float64(T):
    rng = np.random.default_rng(T)
    x = (rng.standard_normal((T, 1024)) * tw.levels(T)[:, None]).astype(np.float32).ravel()
    X = tw.fft_pair_twin(x, T)
    assert X.dtype == np.complex64 and X.shape == (T, 513)
    c, level = tw.fft_figures(X, tw.fft_truth(x, T))
    assert tw.c_max(c) <= 1e-6
    assert tw.c_max(c) >= 1e-8


def test_fft_twin_silent_track_beside_a_loud_one_is_not_silent():
    rng = np.random.default_rng(3)
    x = np.zeros((4, 1024), np.float32)
    x[0] = rng.standard_normal(1024)
    X = tw.fft_pair_twin(x.ravel(), 4)
    peak = np.abs(X[0]).max()
    assert 1e-8 * peak <= np.abs(X[1]).max() <= 1e-6 * peak
    assert not X[2:].any()
