"""The spectrum plan's restatement (spectrum_twin.py) held without a GPU: the counts against brute force, the framing
against the whole stream, known answers (one-hot windows, a sine on a bin, a constant, Hann's overlap sum), the band
sums, the two rules, and the twin's own error on the inputs and under the caps that test_spectrum_gpu.py uses."""
import math

import numpy as np
import pytest

import conv_pair_twin as tw
import spectrum_twin as st

N, BINS = st.N, st.BINS
GRID_B, GRID_H = (1, 64, 100, 512, 1536), (32, 96, 256, 512, 1000, 1024)
TRACKS = [1, 2, 3, 9, 17]


def plan_counts():
    from gpuaudiobench_amd import SpectrumPlan
    return SpectrumPlan.counts


# ---- counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", GRID_H)
@pytest.mark.parametrize("B", GRID_B)
def test_counts_against_brute_force(B, H):
    n = max(40, 3 * H // B + 3)
    ends = [j * H for j in range(1, n * B // H + 2)]
    brute = [sum(1 for e in ends if k * B < e <= (k + 1) * B) for k in range(n)]
    assert st.counts(B, H, 0, n) == brute
    assert plan_counts()(B, H, 0, n) == brute
    assert plan_counts()(B, H, 7, n - 7) == brute[7:]
    assert sum(brute) == n * B // H
    for m in (1, 2, 5):                                   # calls of m buffers: the sum, and under the capacity
        got = [st.count(k * B, m * B, H) for k in range(0, n - m, m)]
        assert got == [sum(brute[k:k + m]) for k in range(0, n - m, m)]
        assert max(got) <= st.capacity(B, H, m) and min(got) >= st.capacity(B, H, m) - 1
    assert max(st.count(p, B, H) for p in range(H)) == st.capacity(B, H, 1)      # some position reaches it
    assert st.frame_ends(0, n * B, H) == [e for e in ends if e <= n * B]


# ---- framing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 96, 256, 1000, 1024])
def test_any_cut_of_a_stream_gives_the_frames_of_the_whole_stream(H):
    T, total = 3, 3072
    x = st.noise(T, total, seed=5)
    w = st.window_hann()
    whole = st.windowed(x, st.frame_ends(0, total, H), w)
    assert len(whole) == total // H
    for B in (1, 64, 96, 512, 1536):
        fr = st.Framer(T, B, H, w)
        got = [fr.take(b) for b in st.blocks(x, B)]
        assert [len(g) for g in got] == st.counts(B, H, 0, total // B)
        assert np.array_equal(np.concatenate(got), whole), B
        assert np.array_equal(fr.hist, x[:, -st.HIST:]) or total < st.HIST
        # the same in calls of unequal numbers of buffers
        fr.reset()
        bl, got, i = st.blocks(x, B), [], 0
        for m in (1, 3, 2, 5, 1) * (len(bl) // 12 + 1):
            if i >= len(bl):
                break
            got.append(fr.take(bl[i:i + m]))
            i += m
        assert np.array_equal(np.concatenate(got), whole), B
    fr = st.Framer(T, 7, H, w)
    for b in st.blocks(x[:, :7 * 40], 7):                 # a short history: the row shifts
        fr.take(b)
    assert np.array_equal(fr.hist[:, -280:], x[:, :280]) and not fr.hist[:, :-280].any()


@pytest.mark.parametrize("n0", [0, 1, 511, 1023])
def test_one_hot_windows_pick_one_sample(n0):
    """A one-hot window at n0 leaves x[jH - N + n0] times a unit phasor: the framing's known answer."""
    T, total, H = 3, 2048, 96
    x = st.noise(T, total, seed=20 + n0, lv=np.ones(T))
    ends = st.frame_ends(0, total, H)
    fr = st.Framer(T, 100, H, st.one_hot(n0))
    frames = np.concatenate([fr.take(b) for b in st.blocks(x[:, :2000], 100)])
    ends = [e for e in ends if e <= 2000]
    assert len(frames) == len(ends)
    want = st.one_hot_answer(x, ends, n0)
    X64, X = st.truth(frames), st.spectra(frames)
    level = np.abs(want).max(axis=-1)
    assert (level[ends.index(1056):] > 0).all()           # frames that start past sample 0 pick a real sample
    assert np.abs(X64 - want).max() <= 1e-12 * level.max()
    lv = np.stack([tw.pair_level(l) for l in level])
    assert (np.abs(X - want).max(axis=-1) <= 4e-6 * lv).all()


# ---- known readings --------------------------------------------------------------------------------------------------
def test_a_sine_on_a_bin_reads_its_amplitude_squared_and_a_constant_its_square():
    w = st.window_hann()
    S = st.window_sum(w)
    assert abs(S - 512.0) <= 1e-5                          # (not 512 exactly: the sum of the rounded values)
    n = np.arange(2 * N)
    for b, A in ((1, 1.0), (37, 0.25), (256, 3.0), (511, 2.0 ** -10)):
        x = (A * np.sin(2 * np.pi * b * n / N + 0.3)).astype(np.float32)[None, :]
        P = st.powers(st.spectra(st.windowed(x, [N, 2 * N], w)), S)
        assert np.allclose(P[:, 0, b], A * A, rtol=2e-6), (b, P[:, 0, b])
        others = np.delete(P[:, 0], [b - 1, b, b + 1], axis=-1)
        assert others.max() <= 1e-10 * A * A               # Hann spreads a bin-centred sine over three bins only
    for c in (1.0, -0.5, 2.0 ** -12):
        x = np.full((1, 2 * N), c, np.float32)
        P = st.powers(st.spectra(st.windowed(x, [N, 2 * N], w)), S)
        assert np.allclose(P[:, 0, 0], c * c, rtol=2e-6) and P[:, 0, 2:].max() <= 1e-10 * c * c
    # the alternating sequence: bin 512 reads c^2 by the same factor as bin 0
    x = (0.5 * np.where(n % 2 == 0, 1.0, -1.0)).astype(np.float32)[None, :]
    P = st.powers(st.spectra(st.windowed(x, [N], w)), S)
    assert np.allclose(P[0, 0, 512], 0.25, rtol=2e-6)


def test_hann_at_hop_256_sums_to_a_constant():
    w = st.window_hann().astype(np.float64)
    tot = np.zeros(N + 3 * 256)
    for j in range(4):
        tot[j * 256:j * 256 + N] += w
    assert np.abs(tot[768:1024] - 2.0).max() <= 2e-7      # four overlapping windows: 4 x 0.5
    assert np.abs(w[:512] + w[512:] - 1.0).max() <= 1e-7   # and hop 512 sums to 1


# ---- bands -----------------------------------------------------------------------------------------------------------
def test_band_sums_against_fsum_within_the_bound_of_an_ordered_sum():
    T = 3
    x = st.noise(T, 2048, seed=9)
    S = st.window_sum(st.window_hann())
    P = st.powers(st.spectra(st.windowed(x, [1024, 1536, 2048], st.window_hann())), S)
    from gpuaudiobench_amd import spectrum_band_edges
    for edges in (st.default_edges(1), st.default_edges(64), spectrum_band_edges(31), [3, 4, 100, 500]):
        got = st.band_sums(P, edges)
        assert got.shape == P.shape[:-1] + (len(edges) - 1,)
        for f in range(P.shape[0]):
            for t in range(T):
                for b in range(len(edges) - 1):
                    vals = [float(v) for v in P[f, t, edges[b]:edges[b + 1]]]
                    assert abs(float(got[f, t, b]) - math.fsum(vals)) <= st.ordered_sum_bound(vals), (f, t, b)
    assert np.array_equal(st.band_sums(P, list(range(BINS + 1))), P)      # a band per bin is the bin


def test_default_and_logarithmic_edges_satisfy_the_rule_for_every_band_count():
    from gpuaudiobench_amd import spectrum_band_edges
    for bands in range(1, 65):
        e = st.default_edges(bands)
        assert st.bad_edge(e, bands) == -1 and e[0] == 0 and e[-1] == BINS
        for args in ((), (48000.0, 20.0, 20000.0), (44100.0, 31.5, None), (48000.0, 1.0, 24000.0),
                     (48000.0, 20000.0, 24000.0)):
            g = spectrum_band_edges(bands, *args)
            assert len(g) == bands + 1 and st.bad_edge(g, bands) == -1, (bands, args, g)
    third = spectrum_band_edges(31)                        # 31 bands over ten octaves: about a third of an octave
    assert third[-1] == BINS and third[0] <= 1
    wide = [b for b in range(31) if third[b + 1] - third[b] > 2]
    ratios = [third[b + 1] / third[b] for b in wide[1:]]
    assert all(1.1 < r < 1.5 for r in ratios), ratios


# ---- the rules -------------------------------------------------------------------------------------------------------
def test_the_edge_rule_on_every_spoilt_field():
    for bands in (1, 5, 64):
        good = st.default_edges(bands)
        assert st.bad_edge(good, bands) == -1
        for b in range(bands + 1):
            for v, first in ((-1, b), (BINS + 1, b), (good[b - 1] if b else -1, b),
                             (good[b + 1] if b < bands else BINS + 1, b if b == bands else b + 1)):
                e = list(good)
                e[b] = v
                got = st.bad_edge(e, bands)
                assert got == (b if v < 0 or v > BINS else first), (bands, b, v, got)
    assert st.bad_edge([0, BINS], 1) == -1 and st.bad_edge([BINS - 1, BINS], 1) == -1
    assert st.bad_edge([5, 5], 1) == 1 and st.bad_edge([6, 5], 1) == 1


def test_the_window_rule_on_every_spoilt_field():
    w = st.window_hann()
    assert st.bad_window(w) is None
    for n in (0, 1, 63, 64, 511, 1023):
        for v in (np.nan, np.inf, -np.inf):
            s = w.copy()
            s[n] = v
            assert st.bad_window(s) == n
    s = w.copy()
    s[[700, 3]] = np.nan
    assert st.bad_window(s) == 3                           # the first
    assert st.bad_window(np.zeros(N, np.float32)) == "sum"
    alt = np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.float32)
    assert st.bad_window(alt) == "sum"
    assert st.bad_window(st.one_hot(5)) is None
    assert st.bad_window(-w) is None                       # a negative sum is a sum


# ---- the twin's own error --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TRACKS)
def test_the_twins_error_is_within_its_cap(T):
    """c_twin on Hann-windowed noise at conv_pair_twin.levels(T): inside (0, 1e-6], so four times it is a bound on the
    kernel that means something (0.9e-7 .. 1.75e-7 measured)."""
    x = st.noise(T, 4096, seed=100 + T)
    frames = st.windowed(x, st.frame_ends(0, 4096, 512), st.window_hann())
    c, level = st.figures(st.spectra(frames), st.truth(frames))
    c_twin = tw.c_max(c)
    print("\nspectrum twin T %d c_twin %.3g" % (T, c_twin))
    assert 0 < c_twin <= 1e-6
    assert (level > 0).all()                               # levels(T) has silent tracks but no silent pair
    # the power bound of test_spectrum_gpu.py is met by the twin itself with the twin's own d
    S = st.window_sum(st.window_hann())
    X64 = st.truth(frames)
    ik = st.inv_k(S).astype(np.float64)
    P64 = np.abs(X64) ** 2 * ik
    d = (c_twin * level)[..., None]
    bound = ik * (2 * np.abs(X64) * d + d * d) + 2.0 ** -22 * P64
    assert (np.abs(st.powers(st.spectra(frames), S).astype(np.float64) - P64) <= bound).all()
