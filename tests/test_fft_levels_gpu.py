"""gab_fft_r2c_1024 held per track.  The kernel packs tracks 2q and 2q + 1 into one complex 1024-point transform (one
per wave, four waves = eight tracks per workgroup; an odd last track beside zeros), so a track's rounding error
follows its pair's spectral peak.  Track counts 1, 2, 3, 9, 17: an odd last track, and the crossing of the 8-track
workgroup.  Per track

    c_t = max over bins |X_t - rfft64(x_t)| / (peak_t + peak_p)  <=  4 c_twin

with c_twin the same figure of the packed float32 restatement (conv_pair_twin.fft_pair_twin) on the same input, and
known answers (impulses, DC, the alternating sequence, cosines on a bin) whose off-peak bins are held in the same
way: leakage relative to the pair's spectral peak (under KNOWN_FACTOR c_twin: see there why not 4)."""
import numpy as np
import pytest

import conv_pair_twin as tw
from test_conv_plan_state_gpu import dev, gab, host, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

TRACKS = [1, 2, 3, 9, 17]
N = 1024


def gpu_fft(gab, x, T):
    y = host(gab.fft_r2c_1024(dev(np.asarray(x, np.float32).ravel()), T)).astype(np.float64)
    return y[..., 0] + 1j * y[..., 1]


def held(gab, x, T, what, factor=4.0):
    """The kernel's spectrum of x [T, 1024], every track within `factor` c_twin of float64 over its pair's peak."""
    x = np.asarray(x, np.float32).ravel()
    truth = tw.fft_truth(x, T)
    ct, level = tw.fft_figures(tw.fft_pair_twin(x, T), truth)
    X = gpu_fft(gab, x, T)
    cg, _ = tw.fft_figures(X, truth)
    c_twin = tw.c_max(ct)
    print("\nfft %s T %d c_twin %.3g c_gpu %.3g ratio %.2f" % (what, T, c_twin, tw.c_max(cg), tw.c_max(cg) / c_twin))
    assert 0 < c_twin <= 1e-6
    assert (level > 0).all()                                         # (silent pairs: test_a_silent_pair_gives_zeros)
    assert (cg <= min(factor * c_twin, 1e-5)).all(), (what, T, cg / c_twin)
    return X, truth


@pytest.mark.parametrize("T", TRACKS)
def test_every_track_is_within_4_c_twin_of_its_pairs_peak(gab, T):
    rng = np.random.default_rng(100 + T)
    x = rng.standard_normal((T, N)) * tw.levels(T)[:, None]
    held(gab, x, T, "levels")


# The known answers: 1.5 x the measured 4.86.  An impulse's spectrum is the bare product of the three passes' twiddles,
# which the kernel forms in registers from one table entry per pass (gab_fft.hpp powers_of: up to four chained products
# per power); scipy reads each from a table rounded once and is nearly exact on an impulse (7.6e-8), while the kernel
# loses what it loses on noise (3.4e-7 of the pair's peak, at n = 511, 512, 1023: the high powers; 6e-8 at n = 0, 1).
# profiles/r18_conv_levels.txt.  On noise the kernel is inside the factor 4 (at most 3.21), and so is the one-track case
# of the known answers (an impulse at n = 1: 0.87), which stays at 4.
KNOWN_FACTOR = 7.3


@pytest.mark.parametrize("T", TRACKS)
def test_known_answers(gab, T):
    """conv_pair_twin.fft_known_answers: impulses at n = 0, 1, 511, 512, 1023, DC, the alternating sequence, cosines
    on bins 1, 255, 256, 511, every spectral peak 1.  Held to float64 under KNOWN_FACTOR c_twin over the pair's peak in
    EVERY bin: off-peak bins are leakage relative to the pair's spectral peak.  The closed forms are held as well
    (4e-6 of the pair's peak: the cosines' float32 samples are 6e-8 off the closed form's)."""
    x, want = tw.fft_known_answers(T)
    X, truth = held(gab, x, T, "known answers", KNOWN_FACTOR if T > 1 else 4.0)
    level = tw.pair_level(np.abs(truth).max(axis=1))
    assert (np.abs(X - want).max(axis=1) <= 4e-6 * level).all()


@pytest.mark.parametrize("T", [9, 17])
def test_a_silent_pair_gives_zeros(gab, T):
    """A whole pair of zeros beside loud pairs (pair 1, in the first workgroup; pair 5 of T = 17, in the second) and an
    odd last track of zeros beside its zero partner: their spectra are zeros, of either sign.  A silent track with a
    loud partner (track 1) is not."""
    rng = np.random.default_rng(400 + T)
    x = rng.standard_normal((T, N)).astype(np.float32)
    silent = [2, 3, T - 1] + ([10, 11] if T > 11 else [])
    x[silent] = 0.0
    x[1] = 0.0
    X = gpu_fft(gab, x, T)
    assert not X[silent].any()
    assert X[1].any() and np.abs(X[1]).max() <= 1e-5 * np.abs(X[0]).max()
    loud = [t for t in range(T) if t not in silent and t != 1]
    assert (np.abs(X[loud] - tw.fft_truth(x.ravel(), T)[loud]).max(axis=1) <= 1e-5 * np.abs(X[loud]).max()).all()


@pytest.mark.parametrize("T", [9, 17])
def test_a_pair_depends_on_nothing_outside_itself(gab, T):
    rng = np.random.default_rng(200 + T)
    x = (rng.standard_normal((T, N)) * tw.levels(T)[:, None]).astype(np.float32)
    x2 = (rng.standard_normal((T, N)) * 2.0 ** 10).astype(np.float32)
    base = host(gab.fft_r2c_1024(dev(x.ravel()), T))
    for q in range((T + 1) // 2):
        own = [t for t in (2 * q, 2 * q + 1) if t < T]
        v = x2.copy()
        v[own] = x[own]
        got = host(gab.fft_r2c_1024(dev(v.ravel()), T))
        assert same_bits(got[own], base[own]), q


@pytest.mark.parametrize("T", TRACKS)
def test_a_nan_stays_in_its_pair_and_reaches_its_partner(gab, T):
    rng = np.random.default_rng(300 + T)
    x = rng.standard_normal((T, N)).astype(np.float32)
    base = host(gab.fft_r2c_1024(dev(x.ravel()), T))
    for t, v in ((0, np.nan), (T - 1, np.inf)):
        d = x.copy()
        d[t, 700] = v
        got = host(gab.fft_r2c_1024(dev(d.ravel()), T))
        pair = [u for u in (t & ~1, (t & ~1) + 1) if u < T]
        for u in range(T):
            if u in pair:
                assert not np.isfinite(got[u]).all(), u              # the struck track and its partner
            else:
                assert same_bits(got[u], base[u]), u
