"""The resample plan's contract restated in numpy (include/gab_c_api.h, gab_resample_*), without a GPU: the tap table
in float64 and rounded once (resample_taps64 / resample_taps32), a whole stream through the ordered one-rounding chain
(resample_reference_f32) and in float64 (resample_reference_f64), a Twin of the plan's state machine with history,
k mod period, counts and zero fill, and known answers that do not trust the restatement.  tests/test_resample_gpu.py
holds the device to these."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mix_host import fma32 as _fma32_finite  # noqa: E402

F32 = np.float32
EPS = 2.0 ** -24
#          up   down
DESIGNED = [(160, 147), (147, 160), (2, 1), (1, 2), (3, 2), (1, 1), (4, 6)]     # run at their default taps
# Ratios whose position arithmetic the designed ones do not reach, with the taps they are run at (the default would
# pass 256 for most): M/L >= 2 with M mod L != 0 (2/5, 7/3, 3/64), K mod 4 = 2 beside M mod L = 2 (5/2), chunks and
# whole buffers without an output (3/200, 1/65, 1/1024), the largest table (64/1), a ratio that reduces (1000/1024).
TAPS = {(2, 5): 16, (5, 2): 6, (7, 3): 12, (3, 200): 8, (3, 64): 64, (1, 65): 8, (1, 1024): 4, (64, 1): 256,
        (1000, 1024): 16}
RATIOS = DESIGNED + sorted(TAPS)


def fma32(a, b, c):
    """fmaf: one rounding.  Where a value is not finite the float64 expression has fmaf's infinity or NaN."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    if fin.all():
        return _fma32_finite(a, b, c)
    with np.errstate(invalid="ignore", over="ignore"):
        rough = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
        z = np.zeros_like(a)
        exact = _fma32_finite(np.where(fin, a, z), np.where(fin, b, z), np.where(fin, c, z))
    return np.where(fin, exact, rough).astype(F32)


def reduced(up, down):
    g = math.gcd(up, down)
    return up // g, down // g


def default_taps(up, down):
    """The smallest multiple of 8 that is at least 32 max(1, M / L)."""
    L, M = reduced(up, down)
    k = 8
    while k * L < 32 * max(L, M):
        k += 8
    return k


def taps_of(up, down):
    """The taps a ratio of RATIOS is run at."""
    return TAPS.get((up, down)) or default_taps(up, down)


def resample_taps64(up, down, K):
    """[L][K] float64: every phase row divided by its sum, added in ascending j."""
    L, M = reduced(up, down)
    pi = 3.14159265358979323846
    c = 0.94 * min(1.0, L / M)
    half = float(K // 2)
    out = np.zeros((L, K))
    for p in range(L):
        h = []
        for j in range(K):
            d = float(j - K // 2) + p / L
            u = d / half
            x = c * d
            s = 1.0 if x == 0.0 else math.sin(pi * x) / (pi * x)
            wnd = 0.35875 + 0.48829 * math.cos(pi * u) + 0.14128 * math.cos(2.0 * pi * u) + \
                0.01168 * math.cos(3.0 * pi * u)
            h.append(s * wnd)
        total = 0.0
        for v in h:
            total += v
        out[p] = [v / total for v in h]
    return out


def resample_taps32(up, down, K):
    return resample_taps64(up, down, K).astype(F32)


def lo(k, B, L, M):
    """The first output of buffer k: ceil(k B L / M), in exact integers."""
    return -(-(k * B * L) // M)


def period_of(B, L, M):
    return M // math.gcd(B * L, M)


def chain(w, taps, I, P, exact):
    """w [T][N + K - 1]: the stream with K-1 earlier samples in front, so that w[:, K-1+s] is sample s.  Outputs at
    newest sample I[n], phase P[n]: [T][n].  exact: float32, the product first, then ascending j, one rounding each."""
    K = taps.shape[1]
    I, P = np.asarray(I, np.int64), np.asarray(P, np.int64)
    if exact:
        w, taps = np.asarray(w, F32), np.asarray(taps, F32)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (taps[P, 0][None, :] * w[:, I + K - 1]).astype(F32)
            for j in range(1, K):
                y = fma32(taps[P, j][None, :], w[:, I + K - 1 - j], y)
        return y
    w, taps = np.asarray(w, np.float64), np.asarray(taps, F32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = taps[P, 0][None, :] * w[:, I + K - 1]
        for j in range(1, K):
            y = taps[P, j][None, :] * w[:, I + K - 1 - j] + y
    return y


def _whole(x, up, down, K, taps, exact):
    L, M = reduced(up, down)
    x = np.atleast_2d(np.asarray(x, F32))
    T, N = x.shape
    taps = resample_taps32(up, down, K) if taps is None else np.asarray(taps, F32).reshape(L, K)
    m = np.arange(lo(1, N, L, M), dtype=np.int64)                    # all outputs whose newest sample is below N
    w = np.concatenate([np.zeros((T, K - 1), F32), x], axis=1)
    return chain(w, taps, (m * M) // L, (m * M) % L, exact)


def resample_reference_f32(x, up, down, K, taps=None):
    """x [T][N], a whole stream from a reset: every output whose newest tap lies in it, [T][ceil(N L / M)] float32."""
    return _whole(x, up, down, K, taps, True)


def resample_reference_f64(x, up, down, K, taps=None):
    return _whole(x, up, down, K, taps, False)


class Twin:
    """The plan's state machine: history, k mod period, counts, zero fill.  exact=True: float32 (the device's bits)."""

    def __init__(self, tracks, bufsize, up, down, K=None, exact=True, first_buffer=0):
        self.T, self.B, self.exact = tracks, bufsize, exact
        self.L, self.M = reduced(up, down)
        self.K = default_taps(up, down) if K is None else K
        self.out_capacity = -(-(bufsize * self.L) // self.M)
        self.period = period_of(bufsize, self.L, self.M)
        self.taps = resample_taps32(up, down, self.K)
        self.reset()
        self.k = first_buffer % self.period

    def reset(self):
        self.hist = np.zeros((self.T, self.K - 1), F32)
        self.k = 0

    def set_taps(self, t):
        self.taps = np.array(t, F32).reshape(self.L, self.K)

    def count(self):
        return lo(self.k + 1, self.B, self.L, self.M) - lo(self.k, self.B, self.L, self.M)

    def process(self, x):
        """x [T][B] -> (rows [T][out_capacity], n_out)."""
        x = np.asarray(x, F32).reshape(self.T, self.B)
        B, L, M, k = self.B, self.L, self.M, self.k
        m = np.arange(lo(k, B, L, M), lo(k + 1, B, L, M), dtype=np.int64)
        pos = m * M - k * B * L                                        # in [0, B L): relative to the buffer's start
        w = np.concatenate([self.hist, x], axis=1)
        rows = np.zeros((self.T, self.out_capacity), F32 if self.exact else np.float64)
        if len(m):
            rows[:, :len(m)] = chain(w, self.taps, pos // L, pos % L, self.exact)
        self.hist = w[:, B:]
        self.k = (k + 1) % self.period
        return rows, len(m)


def noise(n, T, B, seed=7):
    return np.random.RandomState(seed).uniform(-1, 1, (n, T, B)).astype(F32)


def design_figures(up, down, K):
    """(passband ripple in dB over 0 .. 0.8 of the lower Nyquist, largest response in dB from 1.2 of it upward) of the
    float32 table: the prototype filter g[j L + p] = h_p[j] at L times the input rate, by a zero-padded transform."""
    L, M = reduced(up, down)
    g = resample_taps32(up, down, K).astype(np.float64).T.reshape(-1)
    N = 1 << 21
    G = np.abs(np.fft.rfft(g, N)) / L
    f = np.arange(N // 2 + 1) * (L / N)                              # cycles per input sample
    nyq = 0.5 * min(1.0, L / M)
    ripple = np.max(np.abs(20 * np.log10(G[f <= 0.8 * nyq])))
    stop = 20 * np.log10(np.max(G[f >= 1.2 * nyq]))
    return float(ripple), float(stop)


# ---------------------------------------------------------------------------------------------------------------------

def test_counts_over_a_period():
    for up, down in RATIOS:
        L, M = reduced(up, down)
        for B in (1, 7, 31, 64, 100, 513):
            per = period_of(B, L, M)
            twin = Twin(1, B, up, down, K=4)
            assert twin.period == per and twin.out_capacity == -(-(B * L) // M)
            counts = []
            for _ in range(2 * per):
                counts.append(twin.count())
                twin.k = (twin.k + 1) % per
            assert counts[:per] == counts[per:]
            assert sum(counts[:per]) * M == per * B * L                      # exactly period B L / M
            assert set(counts) <= {(B * L) // M, -(-(B * L) // M)}
    assert reduced(4, 6) == (2, 3)


def test_bufsize_one_upsampled_by_two_and_halved():
    from gpuaudiobench_amd import ResamplePlan
    assert ResamplePlan.counts(1, 1, 2, 0, 4) == [1, 0, 1, 0]
    assert ResamplePlan.counts(1, 2, 1, 0, 3) == [2, 2, 2]
    twin = Twin(1, 1, 1, 2, K=4)
    got = [twin.process(np.zeros((1, 1), F32))[1] for _ in range(4)]
    assert got == [1, 0, 1, 0]


def test_plan_counts_agree_with_the_twin_from_any_first_buffer():
    from gpuaudiobench_amd import ResamplePlan
    for up, down in RATIOS:
        for B in (1, 7, 100):
            for first in (0, 1, 5, 1000003):
                twin = Twin(1, B, up, down, K=4, first_buffer=first)
                want = []
                for _ in range(9):
                    want.append(twin.count())
                    twin.k = (twin.k + 1) % twin.period
                assert ResamplePlan.counts(B, up, down, first, 9) == want
    assert ResamplePlan.default_taps(147, 160) == 40 and ResamplePlan.default_taps(160, 147) == 32
    assert ResamplePlan.default_taps(1, 2) == 64 and ResamplePlan.default_taps(2, 1) == 32
    for up, down in RATIOS:
        assert ResamplePlan.default_taps(up, down) == default_taps(up, down)
    assert default_taps(1, 1024) == 32768 and default_taps(64, 1) == 32


def test_a_run_from_ten_periods_and_three_equals_one_from_three():
    for up, down, B in ((160, 147, 7), (147, 160, 31), (3, 2, 5)):
        xs = noise(6, 2, B, seed=B)
        a = Twin(2, B, up, down, first_buffer=3)
        b = Twin(2, B, up, down, first_buffer=10 * a.period + 3)
        for x in xs:
            ra, na = a.process(x)
            rb, nb = b.process(x)
            assert na == nb and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))


def test_twin_in_buffers_equals_the_whole_stream():
    """The same stream cut into buffers, bufsize below K-1 included: history and position carry exactly."""
    for up, down in RATIOS:
        K = taps_of(up, down)
        x = noise(1, 2, 120, seed=up)[0]
        whole = resample_reference_f32(x, up, down, K)
        for B in (1, 7, 40):
            twin = Twin(2, B, up, down, K=K)
            parts = []
            for k in range(120 // B):
                rows, n = twin.process(x[:, k * B:(k + 1) * B])
                assert not rows[:, n:].any()
                parts.append(rows[:, :n])
            got = np.concatenate(parts, axis=1)
            assert np.array_equal(got.view(np.uint32), whole[:, :got.shape[1]].view(np.uint32))
            fed = np.concatenate([np.zeros((2, K - 1), F32), x[:, :(120 // B) * B]], axis=1)    # (K - 1 may pass 120)
            assert np.array_equal(twin.hist, fed[:, -(K - 1):])


def test_one_hot_taps_select_input_samples_exactly():
    """Row p is 1.0 at j = (3 p) mod K: output m is w[i - j] exactly, i and p from exact integers."""
    for up, down in RATIOS:
        L, M = reduced(up, down)
        K = 8
        taps = np.zeros((L, K), F32)
        sel = (3 * np.arange(L)) % K
        taps[np.arange(L), sel] = 1.0
        x = noise(1, 2, 90, seed=down)[0]
        y = resample_reference_f32(x, up, down, K, taps)
        for m in range(y.shape[1]):
            i, p = (m * M) // L, (m * M) % L
            src = i - int(sel[p])
            want = x[:, src] if src >= 0 else np.zeros(2, F32)
            assert np.array_equal(y[:, m].view(np.uint32), want.view(np.uint32)), (up, down, m)


def test_constant_input_comes_out_as_that_constant():
    """Row sums are 1 to rounding (K roundings of the taps: within K eps / 2 of 1, asserted); after the latency a
    constant comes out within 4 ulp.  A property of the designed tables at their default taps: DESIGNED."""
    for up, down in DESIGNED:
        K = default_taps(up, down)
        h = resample_taps32(up, down, K)
        sums = h.astype(np.float64).sum(axis=1)
        assert np.max(np.abs(sums - 1.0)) <= K * EPS
        L, M = reduced(up, down)
        c = F32(0.7310585975646973)
        y = resample_reference_f32(np.full((1, 6 * K), c, F32), up, down, K)[0]
        settled = y[-(-(K * L) // M):]                                  # outputs whose K taps all see the constant
        assert len(settled) > K
        assert np.max(np.abs(settled.astype(np.float64) - float(c))) <= 4 * float(np.spacing(c)), (up, down)


@pytest.mark.parametrize("up,down", [(160, 147), (147, 160)])
def test_design_figures(up, down):
    K = default_taps(up, down)
    for taps in sorted({32, K}):
        ripple, stop = design_figures(up, down, taps)
        print("%d/%d K=%d: passband ripple %.3f dB, stopband %.1f dB" % (up, down, taps, ripple, stop))
    ripple, stop = design_figures(up, down, K)
    assert ripple <= 0.3 and stop <= -95.0


@pytest.mark.parametrize("up,down", [(160, 147), (147, 160)])
@pytest.mark.parametrize("frac", [0.05, 0.2, 0.4])
def test_sines(up, down, frac):
    """A sine at `frac` of the lower rate.  float32 against float64: every output within K 2^-24 sum|h_p| peak (K
    roundings, each at most half an ulp of a partial sum that sum|h_p| peak bounds).  float64 against the analytic sine
    delayed by K/2: the gain of phase p at the sine's frequency differs from 1 by at most the passband ripple plus the
    L-1 images, each below the stopband figure: (10^(0.3/20) - 1) + (L - 1) 10^(-95/20)."""
    L, M = reduced(up, down)
    K = default_taps(up, down)
    f = frac * min(1.0, L / M)                                           # cycles per input sample
    n = np.arange(40 * K)
    x = np.sin(2 * np.pi * f * n).astype(F32)[None, :]
    y32 = resample_reference_f32(x, up, down, K)[0].astype(np.float64)
    y64 = resample_reference_f64(x, up, down, K)[0]
    h = resample_taps32(up, down, K).astype(np.float64)
    m = np.arange(len(y64))
    bound = K * EPS * np.abs(h).sum(axis=1)[(m * M) % L] * 1.0
    assert np.all(np.abs(y32 - y64) <= bound)
    t = m * M / L - K / 2.0
    settled = t >= K                                                     # every tap sees the sine
    want = np.sin(2 * np.pi * f * t)
    err = float(np.max(np.abs(y64 - want)[settled]))
    print("%d/%d at %.2f: float64 against the analytic sine %.5f" % (up, down, frac, err))
    assert err <= (10 ** (0.3 / 20) - 1) + (L - 1) * 10 ** (-95 / 20) + 2.0 ** -23   # + the input's own rounding


def test_row_magnitudes_exceed_one():
    """What the header warns of: sum|h_p| reaches about 2.1 (the half-sample phase at a ratio near 1), so an output can
    exceed the input's peak."""
    worst = max(float(np.abs(resample_taps64(up, down, default_taps(up, down))).sum(axis=1).max())
                for up, down in DESIGNED)
    print("largest sum of magnitudes of a row: %.3f" % worst)
    assert 1.5 <= worst <= 2.2


def test_first_and_last_phase_rows_are_pinned():
    """(160, 147, 32): hex literals made by this restatement."""
    h = resample_taps32(160, 147, 32)
    assert h.shape == (160, 32)
    first = [float(v) for v in h[0]]
    last = [float(v) for v in h[-1]]
    assert first == [float.fromhex(v) for v in PIN_FIRST]
    assert last == [float.fromhex(v) for v in PIN_LAST]
    assert h[0, 16] == h[0].max() and np.array_equal(h[0, 1:], h[0, :0:-1])   # phase 0 is symmetric about j = K/2


PIN_FIRST = ["-0x1.414688p-23", "0x1.20e6cap-18", "-0x1.191632p-15", "0x1.29b89ap-13", "-0x1.d1d3ecp-12",
             "0x1.2a3542p-10", "-0x1.4877f8p-9", "0x1.40aef6p-8", "-0x1.1afa36p-7", "0x1.c98070p-7",
             "-0x1.560d94p-6", "0x1.dc5a2ap-6", "-0x1.367d12p-5", "0x1.7c4afep-5", "-0x1.b6cc8cp-5",
             "0x1.ddd054p-5", "0x1.e147b8p-1", "0x1.ddd054p-5", "-0x1.b6cc8cp-5", "0x1.7c4afep-5",
             "-0x1.367d12p-5", "0x1.dc5a2ap-6", "-0x1.560d94p-6", "0x1.c98070p-7", "-0x1.1afa36p-7",
             "0x1.40aef6p-8", "-0x1.4877f8p-9", "0x1.2a3542p-10", "-0x1.d1d3ecp-12", "0x1.29b89ap-13",
             "-0x1.191632p-15", "0x1.20e6cap-18"]
PIN_LAST = ["0x1.2d6346p-18", "-0x1.2016b4p-15", "0x1.2e571ep-13", "-0x1.d648d2p-12", "0x1.2bc396p-10",
            "-0x1.490354p-9", "0x1.40305cp-8", "-0x1.19a888p-7", "0x1.c5de2cp-7", "-0x1.520ff6p-6",
            "0x1.d49c0ep-6", "-0x1.2f8246p-5", "0x1.70164ep-5", "-0x1.a0bb72p-5", "0x1.acb43ep-5",
            "0x1.e1409ep-1", "0x1.07b38ap-4", "-0x1.cce06cp-5", "0x1.887038p-5", "-0x1.3d65e6p-5",
            "0x1.e3f872p-6", "-0x1.59f24ap-6", "0x1.ccff18p-7", "-0x1.1c3470p-7", "0x1.411118p-8",
            "-0x1.47ccf6p-9", "0x1.288702p-10", "-0x1.cd256cp-12", "0x1.24eca4p-13", "-0x1.11d922p-15",
            "0x1.13ee4ap-18", "-0x1.127d48p-23"]


def test_arguments_are_refused_before_any_device_call():
    """Against the built library, without a GPU."""
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for up, down in ((0, 1), (1, 0), (1025, 1), (1, 1025), (-3, 2)):
        assert lib.gab_resample_create(ctypes.byref(h), 4, 512, up, down, 32) == bad
        assert b"up and down" in lib.gab_last_error() and not h.value
    for taps in (2, 5, 33, 258, 0):
        assert lib.gab_resample_create(ctypes.byref(h), 4, 512, 2, 1, taps) == bad
        assert b"taps" in lib.gab_last_error() and not h.value
    assert lib.gab_resample_create(ctypes.byref(h), 4, 512, 1023, 1024, 32) == _capi.GAB_ERR_UNSUPPORTED
    assert b"16384" in lib.gab_last_error() and not h.value
    assert lib.gab_resample_create(ctypes.byref(h), 0, 512, 2, 1, 32) == bad
    assert lib.gab_resample_create(ctypes.byref(h), 4, 0, 2, 1, 32) == bad
    assert lib.gab_resample_create(ctypes.byref(h), 4, (1 << 20) + 1, 2, 1, 32) == bad
    assert lib.gab_resample_create(None, 4, 512, 2, 1, 32) == bad
    n = ctypes.c_int(0)
    assert lib.gab_resample_process(None, None, None, ctypes.byref(n), None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_resample_process_batch(None, None, None, 1, ctypes.byref(n), None) == bad
    assert lib.gab_resample_set_taps(None, None, None) == bad
    assert lib.gab_resample_reset(None, None) == bad
    assert lib.gab_resample_shape(None, None, None, None, None, None) == bad
    assert lib.gab_resample_state(None, None, None, None) == bad
    assert lib.gab_resample_destroy(None) == bad


def test_resample_plan_is_exported():
    import gpuaudiobench_amd as g
    assert g.ResamplePlan._destroy == "gab_resample_destroy" and not hasattr(g.ResamplePlan, "prepare")
