"""The crossover plan (gab_xover_*) without a GPU: the restatement the GPU tests hold the device to, and what holds the
restatement itself to something it was not written from.

    Twin               the contract of include/gab_c_api.h in numpy, float32 with test_mix_host.fma32 (one rounding per
                       written operation), vectorised over tracks, the state carried from call to call.  What
                       xover_kernel must equal bit for bit, bands and states.
    Twin64             the same sequence in float64 for one track, in plain Python floats: the truth for the float32
                       bound, and the object of the magnitude tests.
    xover_first_refused  the rule of a set, restated; rows64 the table in float64, unrounded.

What the twin is held to: the bands of Twin64 sum to an all-pass (|H| = 1 at every bin), band 0 passes DC and band K - 1
passes Nyquist, every band is 6.02 dB down at its split.  None of that is in the recurrence as written; a wrong
topology, a swapped output or a wrong compensating all-pass breaks it.

The bound of float32 against float64 is 2e-6 of the output's peak: a trapezoidal section's rounding noise is white-ish
at about 2^-24 of the signal per operation and is not amplified by 1 / g^2 as the direct form's is.  Measured 1.6e-8 to
4.1e-7 on the four sets with this seed, so the bound leaves a factor of five for other seeds.  Figures: pytest -s.

Everything that touches gpuaudiobench_amd here (crossover_rows, the export, the section count, the argument checks)
fails without the feature; the tests of the twins alone pass on any commit.
"""
import copy
import ctypes
import math

import numpy as np
import pytest

from plan_helpers import bits
from test_mix_host import fma32

FS = 48000.0
K32 = np.float32(np.sqrt(2.0))
K2 = np.float32(2.0) * K32
SETS = [[1000.0], [120.0, 2500.0], [40.0, 400.0, 4000.0], [20.0, 25.0, 23000.0]]


def section_names(K):
    """The sections of a track in the order of the state array."""
    S = K - 1
    names = []
    for j in range(S):
        names += ["A%d" % j, "B%d" % j, "C%d" % j] + ["D%d%d" % (j, m) for m in range(j + 1, S)]
    return names


def rows64(freqs, fs=FS):
    """[S][3] float64, unrounded: the header's formulas."""
    g = np.tan(np.pi * np.asarray(freqs, np.float64) / fs)
    a1 = 1.0 / (1.0 + g * (g + np.float64(K32)))
    return np.stack([a1, g * a1, g * g * a1], axis=-1)


def rows32(freqs, fs=FS):
    return rows64(freqs, fs).astype(np.float32)


def noise(T, n, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, n)).astype(np.float32)


class Twin:
    """rows [T][S][3] float32, state [T][sections][2] float32; process(x [T][n]) -> [K][T][n], any n."""

    def __init__(self, tracks, bufsize, bands):
        self.T, self.B, self.K, self.S = tracks, bufsize, bands, bands - 1
        self.names = section_names(bands)
        self.at = {name: i for i, name in enumerate(self.names)}
        self.rows = None
        self.state = np.zeros((tracks, len(self.names), 2), np.float32)

    def set_splits(self, rows, first_track=0):
        rows = np.asarray(rows, np.float32).reshape(-1, self.S, 3)
        if self.rows is None:
            self.rows = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (self.T, self.S, 1))
        self.rows[first_track:first_track + len(rows)] = rows

    def reset(self):
        self.state[:] = 0.0

    def _section(self, name, split, v0):
        """One sample of section `name` on split `split`'s row, for every track: (v1, v2)."""
        i = self.at[name]
        a1, a2, a3 = (self.rows[:, split, f] for f in range(3))
        ic = self.state[:, i].T.copy()                                # [2][T]
        with np.errstate(all="ignore"):
            v3 = v0 - ic[1]
            v = fma32(np.stack([a2, a3]), v3, np.stack([a1 * ic[0], fma32(a2, ic[0], ic[1])]))
            self.state[:, i] = fma32(np.float32(2.0), v, -ic).T
        return v[0], v[1]

    @staticmethod
    def _high(v0, v1, v2):
        with np.errstate(all="ignore"):
            return fma32(-K32, v1, v0) - v2

    def sample(self, x):
        """x [T] float32 -> [K][T]."""
        r, lows = x, []
        for j in range(self.S):
            bp, l = self._section("A%d" % j, j, r)
            h = self._high(r, bp, l)
            low = self._section("B%d" % j, j, l)[1]
            cb, cl = self._section("C%d" % j, j, h)
            r = self._high(h, cb, cl)
            lows.append(low)
        for j in range(self.S):
            for m in range(j + 1, self.S):
                band = self._section("D%d%d" % (j, m), m, lows[j])[0]
                lows[j] = fma32(-K2, band, lows[j])
        return np.stack(lows + [r])

    def process(self, x):
        x = np.asarray(x, np.float32).reshape(self.T, -1)
        assert self.rows is not None
        out = np.empty((self.K, self.T, x.shape[1]), np.float32)
        for n in range(x.shape[1]):
            out[:, :, n] = self.sample(x[:, n])
        return out


class Twin64:
    """One track, float64, plain Python floats: rows [S][3] as given (float32 rows for the bound, unrounded for the
    magnitude tests)."""

    def __init__(self, rows):
        self.rows = [[float(v) for v in r] for r in np.asarray(rows, np.float64)]
        self.S = len(self.rows)
        self.names = section_names(self.S + 1)
        self.state = {name: [0.0, 0.0] for name in self.names}
        self.k, self.k2 = float(K32), float(K2)

    def _section(self, name, split, v0):
        a1, a2, a3 = self.rows[split]
        st = self.state[name]
        ic1, ic2 = st
        v3 = v0 - ic2
        v1 = a2 * v3 + a1 * ic1
        v2 = a3 * v3 + (a2 * ic1 + ic2)
        st[0] = 2.0 * v1 - ic1
        st[1] = 2.0 * v2 - ic2
        return v1, v2

    def sample(self, x):
        r, lows = x, []
        for j in range(self.S):
            bp, l = self._section("A%d" % j, j, r)
            h = (r - self.k * bp) - l
            lows.append(self._section("B%d" % j, j, l)[1])
            cb, cl = self._section("C%d" % j, j, h)
            r = (h - self.k * cb) - cl
        for j in range(self.S):
            for m in range(j + 1, self.S):
                lows[j] -= self.k2 * self._section("D%d%d" % (j, m), m, lows[j])[0]
        return lows + [r]

    def process(self, x):
        return np.array([self.sample(float(v)) for v in x], np.float64).T       # [K][n]


def xover_first_refused(rows):
    """The index of the first value a set refuses, None if it passes: the rule of gab_c_api.h on the floats of rows."""
    v = np.asarray(rows, np.float32).ravel()
    one = np.float32(1.0)
    for i in range(v.size):
        x, field = v[i], i % 3
        bad = not np.isfinite(x)
        if field == 0:
            bad = bad or not (0.0 < x <= 1.0)
        if field == 1:
            bad = bad or not (0.0 <= x < 1.0)
        if field == 2:
            a1, a2 = v[i - 2], v[i - 1]
            bad = bad or not (0.0 <= x < 1.0)
            with np.errstate(all="ignore"):
                bad = bad or not (abs((fma32(K32, a2, a1) + x) - one) <= np.float32(2.0 ** -20))
                bad = bad or not (abs(fma32(a2, a2, -(a1 * x))) <= np.float32(2.0 ** -18) * (a2 * a2))
        if bad:
            return i
    return None


def rule_slack(rows):
    """(sum, ratio): the two conditions of field 2 as multiples of their limits, the worst over the rows."""
    r = np.asarray(rows, np.float32).reshape(-1, 3)
    a1, a2, a3 = r[:, 0], r[:, 1], r[:, 2]
    s = np.abs((fma32(K32, a2, a1) + a3) - np.float32(1.0)) / np.float32(2.0 ** -20)
    q = np.abs(fma32(a2, a2, -(a1 * a3))) / (np.float32(2.0 ** -18) * (a2 * a2))
    return float(s.max()), float(q.max())


# ---- 1. the topology ------------------------------------------------------------------------------------------------
def test_section_count_and_state_order():
    assert section_names(2) == ["A0", "B0", "C0"]
    assert section_names(3) == ["A0", "B0", "C0", "D01", "A1", "B1", "C1"]
    assert section_names(4) == ["A0", "B0", "C0", "D01", "D02", "A1", "B1", "C1", "D12", "A2", "B2", "C2"]
    import gpuaudiobench_amd as g
    for K in (2, 3, 4):
        S = K - 1
        assert len(section_names(K)) == 3 * S + S * (S - 1) // 2 == g.lib.gab_xover_sections(K) == g.CrossoverPlan.sections(K)
    assert g.lib.gab_xover_sections(1) == 0 and g.lib.gab_xover_sections(5) == 0
    assert float(K2) == 2.0 * float(K32) and K32.view(np.uint32) == 0x3FB504F3
    assert float.fromhex("0x1.6a09e6p+0") == float(K32) == g.ops.XOVER_K32


def impulse_response(freqs, n):
    x = np.zeros(n)
    x[0] = 1.0
    return Twin64(rows64(freqs)).process(x)


@pytest.mark.parametrize("freqs", SETS[:3])
def test_the_bands_sum_to_an_allpass(freqs):
    h = impulse_response(freqs, 8192)
    assert np.abs(h[:, -64:]).max() < 1e-12                           # the response has died inside the transform
    H = np.fft.rfft(h, axis=1)
    worst = np.abs(np.abs(H.sum(axis=0)) - 1.0).max()
    dc, ny = abs(abs(H[0, 0]) - 1.0), abs(abs(H[-1, -1]) - 1.0)
    print("\nsplits %s: | |sum H| - 1 | <= %.2e, band 0 at DC %.2e, band %d at Nyquist %.2e" % (freqs, worst, dc, len(freqs), ny))
    assert worst < 1e-6 and dc < 1e-6 and ny < 1e-6
    # and the other bands pass neither: band 0 is the only one with a DC gain, band K - 1 the only one at Nyquist
    assert np.abs(H[1:, 0]).max() < 1e-6 and np.abs(H[:-1, -1]).max() < 1e-6


def test_close_splits_and_a_split_near_nyquist_sum_to_an_allpass():
    h = impulse_response(SETS[3], 2 ** 16)
    assert np.abs(h[:, -64:]).max() < 1e-9
    H = np.fft.rfft(h, axis=1)
    worst = np.abs(np.abs(H.sum(axis=0)) - 1.0).max()
    print("\nsplits %s over 2^16 points: | |sum H| - 1 | <= %.2e" % (SETS[3], worst))
    assert worst < 1e-6
    assert abs(abs(H[0, 0]) - 1.0) < 1e-6 and abs(abs(H[-1, -1]) - 1.0) < 1e-6


@pytest.mark.parametrize("freqs", SETS[:3])
def test_every_band_is_six_db_down_at_its_split(freqs):
    """A settled sine at split j: band j (its upper edge) and band j + 1 (its lower edge) are both at -6.02 dB."""
    n = 1 << 15                                                       # 40 Hz: 85 time constants before the tail
    t = np.arange(n)
    for j, f in enumerate(freqs):
        y = Twin64(rows64(freqs)).process(np.sin(2.0 * np.pi * f / FS * t))
        tail = slice(n - int(round(8 * FS / f)), n)                   # eight periods, long after the transient
        basis = np.stack([np.sin(2.0 * np.pi * f / FS * t[tail]), np.cos(2.0 * np.pi * f / FS * t[tail])], axis=1)
        for band in (j, j + 1):
            c = np.linalg.lstsq(basis, y[band, tail], rcond=None)[0]
            db = 20.0 * math.log10(math.hypot(c[0], c[1]))
            print("\nsplits %s: band %d at %g Hz: %.4f dB" % (freqs, band, f, db))
            assert abs(db + 6.0206) < 0.01, (freqs, band, db)


@pytest.mark.parametrize("freqs", SETS[:3])
def test_every_band_is_its_cascade_of_butterworth_sections_and_allpasses(freqs):
    """Band j is, written out as biquads: the second-order Butterworth high-pass of every split below it, twice; the
    low-pass of its own split, twice; the second-order all-pass (the low-pass's denominator, reversed, on top) of every
    split above it.  scipy's sections and scipy's filter, nothing of this file's."""
    from scipy import signal
    x = noise(1, 4096, 22)[0].astype(np.float64)
    y = Twin64(rows64(freqs)).process(x)
    S = len(freqs)
    lp = [signal.butter(2, f, "lowpass", fs=FS, output="sos") for f in freqs]
    hp = [signal.butter(2, f, "highpass", fs=FS, output="sos") for f in freqs]
    ap = [np.concatenate([s[:, 5:2:-1], s[:, 3:]], axis=1) for s in lp]
    for j in range(S + 1):
        sos = [hp[i] for i in range(j) for _ in (0, 1)]
        if j < S:
            sos += [lp[j], lp[j]] + [ap[m] for m in range(j + 1, S)]
        want = signal.sosfilt(np.concatenate(sos), x)
        err = np.abs(y[j] - want).max() / np.abs(want).max()
        print("\nsplits %s band %d against its biquad cascade: %.2e of peak" % (freqs, j, err))
        assert err < 1e-6, (freqs, j, err)                            # K32 is sqrt(2) to 2^-25: 3e-8 measured


# ---- 2. float32 against float64 -------------------------------------------------------------------------------------
F32_BOUND = 2e-6


@pytest.mark.parametrize("freqs", SETS)
def test_float32_is_within_the_bound_of_float64(freqs):
    K, n = len(freqs) + 1, 2048
    x = noise(1, n, 20)
    twin = Twin(1, n, K)
    twin.set_splits(rows32(freqs))
    got = twin.process(x)[:, 0].astype(np.float64)
    want = Twin64(rows32(freqs)).process(x[0].astype(np.float64))
    # "of peak" is of the plan's output, the largest sample of the band block: the reading under which the figures the
    # bound was set from (1.3e-7 to 3.4e-7) are the ones measured here.  Of each band's OWN peak the lowest band of a
    # low split reads higher (a 40 Hz band of white noise peaks near 0.1), and is printed beside it.
    err = np.abs(got - want).max(axis=1) / np.abs(want).max()
    own = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
    print("\nsplits %s: float32 against float64, of the output's peak: %s; of the band's own: %s"
          % (freqs, " ".join("%.2e" % e for e in err), " ".join("%.2e" % e for e in own)))
    assert (err < F32_BOUND).all(), err


# ---- 3. streaming ---------------------------------------------------------------------------------------------------
def test_any_cut_into_buffers_gives_the_bits_of_the_whole_stream():
    T, K, n = 3, 4, 400
    rows = np.stack([rows32(f) for f in ([40.0, 400.0, 4000.0], [20.0, 25.0, 23000.0], [300.0, 310.0, 9000.0])])
    x = noise(T, n, 21)
    whole = Twin(T, n, K)
    whole.set_splits(rows)
    want = whole.process(x)
    for B in (1, 63, 64, 65, 200):
        twin = Twin(T, B, K)
        twin.set_splits(rows)
        got = np.concatenate([twin.process(x[:, s:s + B]) for s in range(0, n, B)], axis=2)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(twin.state), bits(whole.state)), B
    # a deep copy taken mid-stream goes on bit for bit
    twin = Twin(T, 100, K)
    twin.set_splits(rows)
    twin.process(x[:, :100])
    fork = copy.deepcopy(twin)
    a, b = twin.process(x[:, 100:]), fork.process(x[:, 100:])
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(want[:, :, 100:]))
    assert np.array_equal(bits(fork.state), bits(whole.state))


# ---- 4. the rule ----------------------------------------------------------------------------------------------------
def test_every_row_of_crossover_rows_passes_the_rule():
    import gpuaudiobench_amd as g
    worst = (0.0, 0.0)
    for fs in (44100.0, 48000.0, 96000.0, 192000.0):
        f = np.geomspace(5.0, 0.499 * fs, 2000)
        rows = g.crossover_rows(f, fs)
        assert rows.shape == (1, 2000, 3) and rows.dtype == np.float32
        assert np.array_equal(bits(rows[0]), bits(rows32(f, fs)))
        assert xover_first_refused(rows) is None, fs
        s, q = rule_slack(rows)
        worst = (max(worst[0], s), max(worst[1], q))
    print("\nhost-made rows use at most %.3f of the sum condition and %.3f of the ratio condition" % worst)
    assert worst[0] <= 1.0 / 8.0 and worst[1] <= 1.0 / 8.0          # the margin of eight the contract states


def test_a_spoilt_row_is_refused_at_its_index():
    good = np.stack([rows32([100.0, 1000.0, 8000.0]), rows32([50.0, 700.0, 20000.0])])      # [2][3][3]
    assert xover_first_refused(good) is None
    flat = good.reshape(-1)
    in_range = (lambda v: 0.0 < v <= 1.0, lambda v: 0.0 <= v < 1.0)
    for i in range(flat.size):
        for how in (lambda v: v * np.float32(1.001), lambda v: -v, lambda v: np.float32(np.nan), lambda v: np.float32(np.inf)):
            bad = flat.copy()
            bad[i] = how(bad[i])
            # a spoilt a1 or a2 that is still within its own range is caught by the a3 that reads it, the end of its row
            want = i - i % 3 + 2 if (i % 3 < 2 and np.isfinite(bad[i]) and in_range[i % 3](bad[i])) else i
            assert xover_first_refused(bad.reshape(good.shape)) == want, (i, bad[i])
    # the edges themselves: g = 0's row passes, a1 = 0 does not
    assert xover_first_refused(np.array([1.0, 0.0, 0.0], np.float32)) is None
    assert xover_first_refused(np.array([0.0, 0.0, 0.0], np.float32)) == 0
    assert xover_first_refused(np.array([0.5, 1.0, 0.0], np.float32)) == 1


# ---- 5. crossover_rows ----------------------------------------------------------------------------------------------
def test_crossover_rows_known_answers_and_refusals():
    import gpuaudiobench_amd as g
    r = g.crossover_rows(1000.0)
    assert r.shape == (1, 1, 3) and r.dtype == np.float32
    # by hand: a1 = 1 / (1 + g (g + K32)) and so on
    gg = math.tan(math.pi * 1000.0 / 48000.0)
    a1 = 1.0 / (1.0 + gg * (gg + float(K32)))
    assert [float(v).hex() for v in r[0, 0]] == [float(np.float32(v)).hex() for v in (a1, gg * a1, gg * gg * a1)]
    assert [float(v).hex() for v in r[0, 0]] == ["0x1.d2bb7c0000000p-1", "0x1.e975c80000000p-5", "0x1.00a5b40000000p-8"]
    assert [float(v).hex() for v in g.crossover_rows(40.0, 44100.0)[0, 0]] == \
        ["0x1.fdf0de0000000p-1", "0x1.73fda80000000p-9", "0x1.0f5bfa0000000p-17"]
    assert g.crossover_rows([120.0, 2500.0]).shape == (1, 2, 3)
    assert g.crossover_rows([[40.0, 400.0, 4000.0], [20.0, 25.0, 23000.0]]).shape == (2, 3, 3)
    assert np.array_equal(g.crossover_rows([[40.0, 400.0, 4000.0]])[0], rows32([40.0, 400.0, 4000.0]))
    for bad in ([2500.0, 120.0], [100.0, 100.0], 0.0, -5.0, 24000.0, [100.0, 30000.0], float("nan"), []):
        with pytest.raises(ValueError):
            g.crossover_rows(bad)
    with pytest.raises(ValueError):
        g.crossover_rows(23000.0, 44100.0)


# ---- 6. arguments, without a GPU ------------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    import gpuaudiobench_amd as g
    lib, bad = g.lib, g._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 2), (4, 0, 2), (4, 64, 1), (4, 64, 5), (-1, 64, 3)):
        assert lib.gab_xover_create(ctypes.byref(h), *args) == bad and not h.value, args
    assert lib.gab_xover_create(ctypes.byref(h), 4, 64, 5) == bad and b"bands must be 2..4" in lib.gab_last_error()
    assert lib.gab_xover_create(None, 4, 64, 2) == bad
    for fn, args in ((lib.gab_xover_destroy, ()), (lib.gab_xover_reset, (None,)), (lib.gab_xover_process, (None, None, None)),
                     (lib.gab_xover_process_batch, (None, None, 1, None)), (lib.gab_xover_set_splits, (None, None)),
                     (lib.gab_xover_set_splits_tracks, (None, 0, 1, None)), (lib.gab_xover_splits, (None, None)),
                     (lib.gab_xover_state, (None, None))):
        assert fn(None, *args) == bad and b"null pointer" in lib.gab_last_error(), fn


def test_crossover_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "CrossoverPlan" in g.__all__ and "crossover_rows" in g.__all__
    assert issubclass(g.CrossoverPlan, g.ops._TrackPlan) and issubclass(g.CrossoverPlan, g.ops._Prepared)
    for name in ("set_splits", "reset", "process", "process_batch", "splits", "state", "prepare", "launch"):
        assert callable(getattr(g.CrossoverPlan, name)), name
