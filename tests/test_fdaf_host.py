"""The fdaf plan's restatement (tests/fdaf_twin.py) held to known answers, without a GPU.

What the float32 restatement reached here (scipy.fft, this file's seeds), beside the conditions it is held to:
    identification  K = 1, mu 0.5, 64 blocks    misalignment -80.7 dB (condition -50), ERLE 77.0 dB (condition 30)
                    K = 2, mu 0.5, 64 blocks    -69.5 dB (condition -45), ERLE 66.1 dB (condition 30)
                    K = 4, mu 1.0, 64 blocks    -60.6 dB (condition -30), ERLE 58.8 dB
                    (the float64 form reaches the same figures to the tenth; K = 1 at mu = 1: +7 dB, it diverges)
    float32 against float64, 16 blocks, relative to the peak of est: 1.7e-7 to 2.1e-7 (mu = 0, taps set, K = 1, 2, 4),
    5.3e-7 and 4.0e-7 (adapting, K = 2 and 4); the condition is 1e-5.
"""
import functools

import numpy as np
import pytest

from fdaf_twin import BINS, BLOCK, F32, FdafTwin, fdaf_params, first_bad_tap, first_refused, not_finite, tap_spectra, taps_of

# (K, mu, blocks): the identification cases, and the misalignment (dB) each must reach; ERLE where it is asked for
CASES = {1: (0.5, 64, -50.0, 30.0), 2: (0.5, 64, -45.0, 30.0), 4: (1.0, 64, -30.0, None)}
EPS = 1e-3


def response(K, seed=11):
    """A decaying random response of 512 K taps, float64: white noise under exp(-n / (128 K)), unit energy."""
    n = np.arange(BLOCK * K)
    h = np.random.default_rng(seed + K).standard_normal(n.size) * np.exp(-n / (128.0 * K))
    return h / np.sqrt((h ** 2).sum())


def echo(K, blocks, seed=5, T=1):
    """(d, x, h): white noise x [T][512 blocks] float32 and d = x through response(K), float64 rounded once."""
    h = response(K)
    x = (0.25 * np.random.default_rng(seed).standard_normal((T, blocks * BLOCK))).astype(F32)
    d = np.stack([np.convolve(xt.astype(np.float64), h)[:xt.size] for xt in x]).astype(F32)
    return d, x, h


def misalignment_db(taps, h):
    taps = np.asarray(taps, np.float64).ravel()
    return 10.0 * np.log10(((taps - h) ** 2).sum() / (h ** 2).sum())


def erle_db(d, err, blocks=4):
    d, err = np.asarray(d, np.float64)[..., -blocks * BLOCK:], np.asarray(err, np.float64)[..., -blocks * BLOCK:]
    return 10.0 * np.log10((d ** 2).sum() / (err ** 2).sum())


@functools.lru_cache(maxsize=None)
def identified(K, wide=False):
    """(d, x, h, err, est, taps) of the identification case K, one track, from zero taps; read only."""
    mu, blocks = CASES[K][:2]
    d, x, h = echo(K, blocks)
    twin = FdafTwin(1, K, wide)
    twin.set_params(np.array([[mu, EPS]], F32))
    err, est = twin.process(d, x)
    out = (d, x, h, err, est, twin.taps())
    for a in out:
        a.setflags(write=False)
    return out


def noise(T, n, seed, scale=0.25):
    return (scale * np.random.default_rng(seed).standard_normal((T, n))).astype(F32)


def decaying_taps(T, K, seed):
    n = np.arange(BLOCK * K)
    return (np.random.default_rng(seed).standard_normal((T, n.size)) * np.exp(-n / (100.0 * K)) * 0.2).astype(F32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def same_state(a, b):
    return all(same(u, v) for u, v in zip(a.state(), b.state()))


# ---- 1. known answers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_one_hot_taps_are_pure_delays(K):
    L = BLOCK * K
    at = sorted({0, 511, 512 % L, L - 1})
    T = len(at)
    h = np.zeros((T, L), F32)
    h[np.arange(T), at] = 1.0
    x = noise(T, 6 * BLOCK, 3)
    twin = FdafTwin(T, K)
    twin.set_taps(h)
    err, est = twin.process(np.zeros_like(x), x)
    for t, delay in enumerate(at):
        want = np.concatenate([np.zeros(delay, F32), x[t, :x.shape[1] - delay]])
        assert np.abs(est[t] - want).max() <= 1e-5 * np.abs(x[t]).max(), (K, delay)
        assert np.abs(err[t] + want).max() <= 1e-5 * np.abs(x[t]).max()


def test_taps_of_set_taps_gives_the_taps_back():
    T, K = 3, 3
    h = decaying_taps(T, K, 8)
    twin = FdafTwin(T, K)
    twin.set_taps(h)
    assert twin.W.dtype == np.complex64 and twin.W.shape == (T, K, BINS)
    assert np.abs(twin.taps() - h).max() <= 4e-7 * np.abs(h).max()
    part = taps_of(tap_spectra(h[1:2], K))
    assert np.array_equal(part, twin.taps()[1:2])                    # a track's spectra depend on its own taps alone


def test_a_new_plan_returns_the_input_and_plus_zero():
    T, K = 3, 2
    d, x = noise(T, 2 * BLOCK, 4, 1e3), noise(T, 2 * BLOCK, 5, 1e3)
    d[0, 3] = -0.0
    twin = FdafTwin(T, K)
    err, est = twin.process(d, x)
    assert np.array_equal(err.view(np.uint32), d.view(np.uint32)) and not est.view(np.uint32).any()
    assert not np.abs(twin.W).max() and (twin.count == 2).all() and same(twin.prev, x[:, BLOCK:])


@pytest.mark.parametrize("K", sorted(CASES))
def test_a_known_response_is_identified(K):
    mu, blocks, condition, erle = CASES[K]
    d, x, h, err, est, taps = identified(K)
    assert err.dtype == F32 and taps.dtype == F32
    assert misalignment_db(taps, h) <= condition, misalignment_db(taps, h)
    if erle is not None:
        assert erle_db(d, err) >= erle, erle_db(d, err)


def test_the_prototype_reaches_its_figures_in_float64():
    """The float64 form of the same steps: -80.7, -69.5 and -60.6 dB here."""
    for K, least in ((1, -65.0), (2, -60.0), (4, -42.0)):
        d, x, h, err, est, taps = identified(K, True)
        assert taps.dtype == np.float64 and misalignment_db(taps, h) <= least, (K, misalignment_db(taps, h))


def test_one_partition_diverges_at_step_one():
    """Why the rule's note says 0.5 for K = 1: at mu = 1 the same case does not converge."""
    d, x, h = echo(1, 64)
    twin = FdafTwin(1, 1, True)
    twin.set_params(np.array([[1.0, EPS]], F32))
    twin.process(d, x)
    assert not misalignment_db(twin.taps(), h) <= -20.0


# ---- 2. the cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_any_cut_into_buffers_and_batches_is_the_whole_stream(K):
    T, blocks = 3, 12
    d, x = noise(T, blocks * BLOCK, 20), noise(T, blocks * BLOCK, 21)
    p = np.array([[0.5, 1e-3], [0.0, 1.0], [0.3, 1e-2]], F32)
    whole = FdafTwin(T, K)
    whole.set_params(p)
    werr, west = whole.process(d, x)
    for B in (512, 1024, 1536):
        n = blocks * BLOCK // B
        ds, xs = (a.reshape(T, n, B).transpose(1, 0, 2) for a in (d, x))
        singles, batched = FdafTwin(T, K), FdafTwin(T, K)
        for t in (singles, batched):
            t.set_params(p)
        outs = [singles.process(ds[i], xs[i]) for i in range(n)]
        berr = np.concatenate([batched.process_batch(ds[:n // 2], xs[:n // 2])[0],
                               batched.process_batch(ds[n // 2:], xs[n // 2:])[0]])
        err = np.concatenate([o[0] for o in outs], axis=1)
        est = np.concatenate([o[1] for o in outs], axis=1)
        assert same(err, werr) and same(est, west) and same(berr.transpose(1, 0, 2).reshape(T, -1), werr), B
        assert same_state(singles, whole) and same_state(batched, whole), B


# ---- 3. containment -----------------------------------------------------------------------------------------------
def spoilt(T, K, blocks=10):
    """(d, x, dirty_d, dirty_x, p, skips): a NaN in track 0's reference in block 2, which lies in the windows of blocks
    2 and 3 and so in the delay line through block K + 2: K + 1 blocks of pair 0; an infinity in track 3's input in
    block 7: one sample, one block of pair 1.  skips[pair]: the blocks whose adaptation that pair loses."""
    d, x = noise(T, blocks * BLOCK, 30), noise(T, blocks * BLOCK, 31)
    d = (d * F32(0.2) + F32(0.5) * np.roll(x, 3, axis=1)).astype(F32)
    p = np.tile(np.array([0.5, 1e-3], F32), (T, 1))
    dirty_d, dirty_x = d.copy(), x.copy()
    dirty_x[0, 2 * BLOCK + 100] = np.nan
    dirty_d[3, 7 * BLOCK + 30] = np.inf
    return d, x, dirty_d, dirty_x, p, {0: set(range(2, K + 3)), 1: {7}}


@pytest.mark.parametrize("K", [1, 3])
def test_what_is_not_finite_stays_in_its_pair_and_out_of_the_taps(K):
    T, blocks = 4, 10
    d, x, dirty_d, dirty_x, p, skips = spoilt(T, K, blocks)
    twin = FdafTwin(T, K)
    twin.set_params(p)
    err, est = twin.process(dirty_d, dirty_x)
    bad = np.zeros((T, blocks * BLOCK), bool)
    bad[0, 2 * BLOCK:(K + 3) * BLOCK] = True                         # (the restatement transforms a track alone: on
    assert np.array_equal(~np.isfinite(est), bad)                    # the device track 1 shares track 0's transforms)
    bad[3, 7 * BLOCK + 30] = True
    assert np.array_equal(~np.isfinite(err), bad)
    assert np.isfinite(twin.W.view(F32)).all() and twin.skipped == K + 2
    # the taps are those of the clean stream with those blocks' adaptation left out, pair by pair
    for pair in (0, 1):
        rows = slice(2 * pair, 2 * pair + 2)
        clean = FdafTwin(2, K)
        clean.set_params(p[rows])
        for b in range(blocks):
            cut = slice(b * BLOCK, (b + 1) * BLOCK)
            clean.process(d[rows, cut], x[rows, cut], adapt=b not in skips[pair])
        assert same(twin.W[rows], clean.W[rows.start - 2 * pair:rows.stop - 2 * pair]), pair
        assert (clean.count == blocks).all()


def test_the_state_after_a_skip():
    """count advances and the constrained partition moves on: the block behind a skipped one constrains the next one."""
    K = 3
    d, x = noise(2, 3 * BLOCK, 40), noise(2, 3 * BLOCK, 41)
    d[1, 10] = np.inf                                               # block 0 is skipped
    twin = FdafTwin(2, K)
    twin.set_params(np.tile(np.array([0.5, 1e-3], F32), (2, 1)))
    twin.set_taps(decaying_taps(2, K, 42))
    before = twin.W.copy()
    twin.process(d[:, :BLOCK], x[:, :BLOCK])
    assert same(twin.W, before) and (twin.count == 1).all() and twin.skipped == 1
    assert same(twin.prev, x[:, :BLOCK]) and np.abs(twin.X[:, 0]).max() > 0 and not np.abs(twin.X[:, 1:]).max()
    twin.process(d[:, BLOCK:2 * BLOCK], x[:, BLOCK:2 * BLOCK])
    tails = np.abs(np.fft.irfft(twin.W.astype(np.complex128), axis=-1)[..., BLOCK:]).max(axis=(0, 2))
    heads = np.abs(np.fft.irfft(twin.W.astype(np.complex128), axis=-1)[..., :BLOCK]).max()
    assert tails[1] <= 1e-6 * heads and tails[0] > 1e-4 * heads, (tails, heads)       # partition 1, not 0 again


# ---- 4. float32 against float64 -----------------------------------------------------------------------------------
# Adapting at K = 2 and 4.  K = 1 at mu = 0.5 stands a factor of two from divergence and multiplies the rounding of a
# bin whose power is nearly nothing: the same run reached 1.9e-5 there (block 12 on), and is no yardstick for a device.
@pytest.mark.parametrize("K,adapting", [(1, False), (2, False), (4, False), (2, True), (4, True)])
def test_float32_is_within_1e_5_of_float64(K, adapting):
    T, blocks = 2, 16
    d, x, _ = echo(K, blocks, seed=50 + K, T=T)                      # an echo: what the adapting filter is for
    p = np.tile(np.array([0.5 if adapting else 0.0, 1e-3], F32), (T, 1))
    outs = []
    for wide in (False, True):
        twin = FdafTwin(T, K, wide)
        twin.set_params(p)
        twin.set_taps(decaying_taps(T, K, 70))
        outs.append(twin.process(d, x))
    peak = np.abs(outs[1][1]).max()
    assert np.abs(outs[0][1] - outs[1][1]).max() <= 1e-5 * peak and np.abs(outs[0][0] - outs[1][0]).max() <= 1e-5 * peak


def test_a_track_that_does_not_adapt_keeps_its_taps_bit_for_bit():
    T, K = 2, 3
    d, x = noise(T, 5 * BLOCK, 80), noise(T, 5 * BLOCK, 81)
    twin = FdafTwin(T, K)
    twin.set_params(np.array([[0.0, 1.0], [0.5, 1e-3]], F32))
    twin.set_taps(decaying_taps(T, K, 82))
    before = twin.W.copy()
    twin.process(d, x)
    assert np.array_equal(twin.W[0].view(F32).view(np.uint32), before[0].view(F32).view(np.uint32))
    assert not same(twin.W[1], before[1])


# ---- 5. the rule and the helper -----------------------------------------------------------------------------------
def test_the_rule_on_every_spoilt_field():
    up = lambda v, to=np.inf: np.nextafter(F32(v), F32(to))            # noqa: E731
    good = np.array([[0.5, 1e-3], [1.0, 2.0 ** -126], [-0.0, 2.0 ** 64], [2.0 ** -149, 1.0]], F32)
    assert first_refused(good) is None
    for (t, f), v in (((0, 0), up(1.0, 2.0)), ((1, 0), np.nan), ((2, 0), np.inf), ((3, 0), -2.0 ** -149), ((0, 1), 0.0),
                      ((1, 1), 2.0 ** -127), ((2, 1), up(2.0 ** 64)), ((3, 1), np.nan), ((0, 1), -1.0), ((1, 0), 2.0)):
        bad = good.copy()
        bad[t, f] = v
        if t + 1 < len(bad):
            bad[t + 1, 1] = np.nan                                    # the FIRST offender is named
        assert first_refused(bad) == 2 * t + f, (t, f, v)
        twin = FdafTwin(4, 1)
        with pytest.raises(ValueError, match="track %d field %d" % (t, f)):
            twin.set_params(bad)
        assert same(twin.params, np.tile(np.array([0.0, 1.0], F32), (4, 1)))
    h = np.zeros((2, 2 * BLOCK), F32)
    h[1, 700] = np.inf
    assert first_bad_tap(h) == 2 * BLOCK + 700
    twin = FdafTwin(3, 2)
    with pytest.raises(ValueError, match="track 2 tap 700"):
        twin.set_taps(h, first_track=1)
    assert not np.abs(twin.W).max()


def test_pinned_rows_of_fdaf_params():
    assert np.array_equal(fdaf_params(), np.array([0.5, 1024e-6], np.float64).astype(F32))
    assert np.array_equal(fdaf_params(1.0, -40.0, 16), np.array([1.0, 16 * 1024 * 1e-4], np.float64).astype(F32))
    assert np.array_equal(fdaf_params(0.25, -90.0, 4).view(np.uint32), np.array([0x3e800000, 0x3689705f], np.uint32))
    assert first_refused(fdaf_params(1.0, -200.0, 1)) is None and first_refused(fdaf_params(1.0, -420.0, 1)) == 1
