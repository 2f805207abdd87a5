"""The matrix-convolution plan's restatement (tests/mconv_twin.py) held to known answers, without a GPU.

What the float32 restatement reached here (scipy.fft, this file's seeds), beside the condition it is held to: float32
against float64 relative to the peak of the output, 1.7e-7 to 3.1e-7 over (I, O, K) = (3, 2, 1), (5, 3, 2), (65, 2, 3);
the condition is 1e-5, the fdaf file's.
"""
import functools
import math

import numpy as np
import pytest

from fdaf_twin import FdafTwin
from mconv_twin import BINS, BLOCK, F32, GROUP, MconvTwin, first_bad_tap, groups, matrix_product, tap_spectra

SHAPES = [(3, 2, 1), (5, 3, 2), (65, 2, 3)]


def noise(I, n, seed, scale=0.25):
    """[I][n] white noise at unequal levels: input i at scale / (1 + i mod 4)."""
    x = np.random.default_rng(seed).standard_normal((I, n)) * (scale / (1.0 + np.arange(I) % 4))[:, None]
    return x.astype(F32)


def decaying_taps(O, I, K, seed):
    n = np.arange(BLOCK * K)
    return (np.random.default_rng(seed).standard_normal((O, I, n.size)) * np.exp(-n / (100.0 * K)) * 0.2).astype(F32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def same_state(a, b):
    return all(same(u, v) for u, v in zip(a.state(), b.state()))


def started(I, O, K, h=None, wide=False):
    twin = MconvTwin(I, O, K, wide)
    if h is not None:
        twin.set_taps(h, ramp=False)
    return twin


def direct(x, h):
    """The float64 truth by definition: y[o] = sum_i x[i] * h[o][i], cut to the stream's length."""
    O, I = h.shape[:2]
    y = np.zeros((O, x.shape[1]))
    for o in range(O):
        for i in range(I):
            y[o] += np.convolve(x[i].astype(np.float64), h[o, i].astype(np.float64))[:x.shape[1]]
    return y


@functools.lru_cache(maxsize=None)
def scenario(I, O, K, blocks=6):
    """(x, h, y of the float32 restatement, y of the float64 one); read only."""
    x, h = noise(I, blocks * BLOCK, 10 + I), decaying_taps(O, I, K, 20 + I)
    out = (x, h, started(I, O, K, h).process(x), started(I, O, K, h, wide=True).process(x))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. known answers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_one_hot_taps_are_pure_delays_on_their_output(K):
    I, O, L = 3, 2, BLOCK * K
    x = noise(I, 6 * BLOCK, 3)
    for delay in sorted({0, 511, 512 % L, L - 1}):
        h = np.zeros((O, I, L), F32)
        h[1, 2, delay] = 1.0                                          # off the diagonal
        y = started(I, O, K, h).process(x)
        want = np.concatenate([np.zeros(delay, F32), x[2, :x.shape[1] - delay]])
        assert np.abs(y[1] - want).max() <= 1e-5 * np.abs(x[2]).max(), (K, delay)
        assert not y[0].view(np.uint32).any()                        # +0 elsewhere


def test_a_new_plan_is_plus_zero():
    twin = MconvTwin(3, 3, 2)
    x = noise(3, 2 * BLOCK, 4, 1e3)
    y = twin.process(x)
    assert y.dtype == F32 and y.shape == (3, 2 * BLOCK) and not y.view(np.uint32).any()
    assert twin.count == 2 and same(twin.prev, x[:, BLOCK:]) and twin.X.shape == (2 + 15, 3, BINS)


@pytest.mark.parametrize("I,O,K", SHAPES)
def test_the_truth_is_the_direct_convolution_summed_over_the_inputs(I, O, K):
    x, h, _, wide = scenario(I, O, K)
    want = direct(x, h)
    assert wide.dtype == np.float64 and np.abs(wide - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("I,O,K", SHAPES)
def test_float32_is_within_1e_5_of_float64(I, O, K):
    _, _, narrow, wide = scenario(I, O, K)
    assert narrow.dtype == F32
    err = np.abs(narrow - wide).max() / np.abs(wide).max()
    print("mconv restatement I=%d O=%d K=%d: float32 against float64 %.2e of peak" % (I, O, K, err))
    assert err <= 1e-5


# ---- 2. the sums ------------------------------------------------------------------------------------------------------
def test_the_group_cut_depends_on_the_inputs_alone():
    assert [list(g) for g in groups(3)] == [[0, 1, 2]]
    assert [(g[0], g[-1]) for g in groups(65)] == [(0, 31), (32, 63), (64, 64)]
    assert [(g[0], g[-1]) for g in groups(64)] == [(0, 31), (32, 63)] and GROUP == 32


def test_the_sums_are_the_tree_as_written_and_within_the_bound_of_an_ordered_sum():
    I, O, K = 70, 2, 3
    rng = np.random.default_rng(6)
    Xs = (rng.standard_normal((K, I, BINS)) + 1j * rng.standard_normal((K, I, BINS))).astype(np.complex64)
    H = (rng.standard_normal((O, I, K, BINS)) + 1j * rng.standard_normal((O, I, K, BINS))).astype(np.complex64)
    Y = matrix_product(Xs, H)
    assert Y.dtype == np.complex64 and Y.shape == (O, BINS)
    eps = 2.0 ** -24
    for o, k in ((0, 0), (1, 7), (0, 512)):
        # (the products row by row, as matrix_product forms them: numpy's product of a row is not bound to be its
        # product of a scalar, bit for bit; the additions are what is held here)
        terms = [[(Xs[p, i] * H[o, i, p])[k] for i in g for p in range(K)] for g in groups(I)]
        partials = []
        for chain in terms:                                           # the tree as written, scalar by scalar
            acc = np.complex64(0)
            for t in chain:
                acc = np.complex64(acc + t)
            partials.append(acc)
        y = partials[0]
        for part in partials[1:]:
            y = np.complex64(y + part)
        assert y == Y[o, k], (o, k)
        # an ordered sum of n terms in any bracketing of depth d: |error| <= d eps sum |t| to first order; the longest
        # path here is a chain of 32 K additions and the two group additions behind it
        flat = [t for chain in terms for t in chain]
        depth = GROUP * K + len(terms) - 1
        for part in (np.real, np.imag):
            exact, size = math.fsum(float(part(t)) for t in flat), math.fsum(abs(float(part(t))) for t in flat)
            assert abs(float(part(y)) - exact) <= 1.01 * depth * eps * size, (o, k)


@pytest.mark.parametrize("n,K", [(1, 1), (2, 2), (3, 3), (5, 2), (34, 1)])
def test_a_diagonal_table_is_the_fdaf_restatement_with_mu_0(n, K):
    x = noise(n, 5 * BLOCK, 30 + n)
    h = decaying_taps(1, n, K, 40 + n)[0]                             # [n][512 K]: track t's taps, on (t, t)
    table = np.zeros((n, n, K * BLOCK), F32)
    table[np.arange(n), np.arange(n)] = h
    fdaf = FdafTwin(n, K)
    fdaf.set_taps(h)
    _, est = fdaf.process(np.zeros_like(x), x)
    y = started(n, n, K, table).process(x)
    assert y.dtype == est.dtype and np.array_equal(y, est)


# ---- 3. the cut, sets, a reset ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,O,K", [(3, 2, 1), (5, 3, 2), (33, 1, 3)])
def test_any_cut_into_buffers_and_batches_is_the_whole_stream(I, O, K):
    x, h = noise(I, 18 * BLOCK, 50), decaying_taps(O, I, K, 51)     # 18 blocks: past the ring's 16 rounds' worth
    whole = started(I, O, K, h)
    want = whole.process(x)
    for B in (512, 1024, 1536):
        n = x.shape[1] // B
        bufs = np.ascontiguousarray(x[:, :n * B].reshape(I, n, B).transpose(1, 0, 2))
        single, batch = started(I, O, K, h), started(I, O, K, h)
        got = np.concatenate([single.process(b) for b in bufs], axis=1)
        two = np.concatenate([batch.process_batch(bufs[:n // 2]), batch.process_batch(bufs[n // 2:])])
        assert same(got, want[:, :n * B]) and same(two.transpose(1, 0, 2).reshape(O, n * B), got)
        assert same_state(single, batch)
        if n * B == x.shape[1]:
            assert same_state(single, whole)


def test_an_unramped_set_mid_stream_is_the_plan_that_had_the_taps_from_the_start():
    I, O, K, B = 5, 3, 2, 1024
    x, h1, h2 = noise(I, 6 * B, 60), decaying_taps(O, I, K, 61), decaying_taps(O, I, K, 62)
    moved, there = started(I, O, K, h1), started(I, O, K, h2)
    for n in range(6):
        if n == 2:
            moved.set_taps(h2, ramp=False)
        a, b = moved.process(x[:, n * B:(n + 1) * B]), there.process(x[:, n * B:(n + 1) * B])
        assert same(a, b) == (n >= 2), n                              # the ring holds input spectra only
    assert same_state(moved, there)


def test_a_ramped_set_is_the_blend_of_the_two_plans():
    I, O, K, B = 5, 3, 2, 1024
    x, h1, h2 = noise(I, 6 * B, 70), decaying_taps(O, I, K, 71), decaying_taps(O, I, K, 72)
    moved, old, new = started(I, O, K, h1), started(I, O, K, h1), started(I, O, K, h2)
    r = ((np.arange(B, dtype=np.float64) + 1.0) / B).astype(F32)
    for n in range(6):
        if n == 2:
            moved.set_taps(h2[1:, 2:], ramp=True, first_output=1, first_input=2)
            moved.set_taps(h2, ramp=True)                             # a second set before the buffer: one ramp
            assert moved.pending and same(moved.current, old.current)
        cut = slice(n * B, (n + 1) * B)
        y, a, b = moved.process(x[:, cut]), old.process(x[:, cut]), new.process(x[:, cut])
        want = a if n < 2 else b if n > 2 else (b - a) * r[None, :] + a
        assert same(y, want), n
    assert not moved.pending and same_state(moved, new) and r[-1] == 1.0


def test_a_ranged_set_is_the_whole_set_of_the_merged_table():
    I, O, K = 5, 3, 2
    h1, h2 = decaying_taps(O, I, K, 80), decaying_taps(O, I, K, 81)
    merged = h1.copy()
    merged[1:3, 2:4] = h2[1:3, 2:4]
    a, b = started(I, O, K, h1), started(I, O, K, merged)
    a.set_taps(h2[1:3, 2:4], ramp=False, first_output=1, first_input=2)
    assert same_state(a, b)
    assert same(tap_spectra(h1[1:2, 2:3], K), tap_spectra(h1, K)[1:2, 2:3])      # a cell's spectra are its own taps'


@pytest.mark.parametrize("K", [1, 3])
def test_what_is_not_finite_leaves_after_k_plus_1_blocks(K):
    I, O, blocks = 3, 2, K + 6
    x, h = noise(I, blocks * BLOCK, 90), decaying_taps(O, I, K, 91)
    h[1, 0] = 0.0                                                     # NaN 0 is NaN: output 1 is not spared
    dirty, zeroed = x.copy(), x.copy()
    dirty[0, 2 * BLOCK + 5], dirty[0, 2 * BLOCK + 300] = np.nan, np.inf
    zeroed[0, 2 * BLOCK + 5] = zeroed[0, 2 * BLOCK + 300] = 0.0
    a, b = started(I, O, K, h), started(I, O, K, h)
    H = a.target.copy()
    for n in range(blocks):
        cut = slice(n * BLOCK, (n + 1) * BLOCK)
        y, want = a.process(dirty[:, cut]), b.process(zeroed[:, cut])
        bad = 2 <= n < 2 + K + 1                                      # the sample lies in two windows
        assert (~np.isfinite(y)).all() == bad and np.isfinite(y).all() == (not bad), n
        if not bad:
            assert same(y, want), n
    assert same(a.target, H) and same(a.current, H)


def test_a_spoilt_tap_is_named_and_changes_nothing():
    I, O, K = 5, 3, 2
    h = decaying_taps(O, I, K, 95)
    twin, ref = started(I, O, K, h), started(I, O, K, h)
    bad = decaying_taps(2, 2, K, 96)
    bad[1, 0, 700], bad[1, 1, 3] = np.inf, np.nan
    assert first_bad_tap(bad) == (1, 0, 700) and first_bad_tap(h) is None
    with pytest.raises(ValueError, match="output 2 input 3 tap 700"):
        twin.set_taps(bad, ramp=True, first_output=1, first_input=3)
    assert same_state(twin, ref) and not twin.pending


def test_a_reset_keeps_the_taps_and_drops_the_ramp():
    I, O, K, B = 3, 2, 2, 512
    x, h1, h2 = noise(I, 4 * B, 97), decaying_taps(O, I, K, 98), decaying_taps(O, I, K, 99)
    used, new = started(I, O, K, h1), started(I, O, K, h2)
    used.process(x[:, :2 * B])
    used.set_taps(h2, ramp=True)
    used.reset()
    assert not used.pending and used.count == 0 and not np.abs(used.X).max() and not np.abs(used.prev).max()
    assert same(used.process(x), new.process(x)) and same_state(used, new)


# ---- 4. the library without a device ----------------------------------------------------------------------------------
def test_the_package_exports_the_plan_and_its_entries():
    import gpuaudiobench_amd as gab
    assert gab.MatrixConvPlan.__name__ in gab.__all__ and gab.MatrixConvPlan.BLOCK == BLOCK and gab.MatrixConvPlan.BINS == BINS
    entries = sorted(n for n in gab._capi.PROTOTYPES if n.startswith("gab_mconv_"))
    assert entries == ["gab_mconv_" + n for n in ("create", "destroy", "process", "process_batch", "reset", "set_taps",
                                                    "set_taps_range", "state")]
    assert all(hasattr(gab.lib, n) for n in entries)


def test_the_refusals_that_come_before_any_device_call():
    """The ranges of create (the twin's limits are the library's) and every entry's null check: no plan is made here."""
    import ctypes
    import gpuaudiobench_amd as gab
    from mconv_twin import MAX_CELLS, MAX_I, MAX_K, MAX_O
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    said = lambda text: text in lib.gab_last_error()                   # noqa: E731
    h = ctypes.c_void_p()
    create = lambda *a: lib.gab_mconv_create(ctypes.byref(h), *a)      # noqa: E731  (inputs, bufsize, outputs, partitions)
    for inputs, bufsize in ((0, 512), (4, 0), (-1, 512)):
        assert create(inputs, bufsize, 2, 1) == bad and not h.value and said(b"tracks and bufsize must be > 0")
    assert create(MAX_I + 1, 512, 1, 1) == bad and not h.value and said(b"inputs must be 1..4096")
    for outputs in (0, -1, MAX_O + 1):
        assert create(4, 512, outputs, 1) == bad and not h.value and said(b"outputs must be 1..64")
    for parts in (0, -1, MAX_K + 1):
        assert create(4, 512, 2, parts) == bad and not h.value and said(b"partitions must be 1..32")
    for inputs, outputs, parts in ((MAX_I, 17, 1), (1025, MAX_O, 1), (64, 64, 17), (MAX_CELLS // 64 + 1, 64, 1)):
        assert inputs * outputs * parts > MAX_CELLS
        assert create(inputs, 512, outputs, parts) == bad and not h.value
        assert said(b"inputs * outputs * partitions must be at most 65536")
    for bufsize in (64, 256, 511, 513, 1000):
        assert create(4, bufsize, 2, 1) == bad and not h.value and said(b"bufsize must be a multiple of 512")
    assert lib.gab_mconv_create(None, 4, 512, 2, 1) == bad and said(b"null plan pointer")
    some = ctypes.c_void_p(64)                                        # never read: the plan is null
    for rc in (lib.gab_mconv_process(None, some, some, None), lib.gab_mconv_process_batch(None, some, some, 2, None),
               lib.gab_mconv_set_taps(None, some, 0, None), lib.gab_mconv_set_taps_range(None, some, 0, 1, 0, 1, 1, None),
               lib.gab_mconv_reset(None, None), lib.gab_mconv_state(None, None, None, None, None, None, None)):
        assert rc == bad and said(b"null pointer")
    assert lib.gab_mconv_destroy(None) == bad and said(b"gab_mconv_destroy: null pointer")
