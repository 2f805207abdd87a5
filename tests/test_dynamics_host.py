"""The dynamics plan (gab_dyn_*) without a GPU: the restatement the GPU tests compare against, held without trusting it.

    dyn_reference_f32  the contract of include/gab_c_api.h in numpy, vectorised over tracks and, outside the smoothing,
                       over samples: every operation a float32 operation rounded once, fma32 (tests/test_mix_host.py)
                       where the contract says fmaf, the coefficients read through gab_dyn_poly.  What dyn_kernel must
                       equal bit for bit.
    dyn_reference_f64  its twin: the same float32 parameters per sample (they are the control path and the contract's),
                       the level, the curve, the smoothing and the gain in float64 with np.log2 / np.exp2.

The a-priori bound of |s32 - s64| (dyn_bound), u = 2^-24, for levels |L| <= Lmax, |thr| <= Tmax, knee <= K,
|slope| <= S, |g| <= G (G <= |range|), att, rel <= A:
  * the level: t r(t) against log2 is held to P = 2^-18 over every mantissa (test_log2_polynomial; the product's
    rounding is inside that figure); adding the exponent is one rounding, u Lmax.                 dL = P + u Lmax
  * over = L - thr: one rounding, u (Lmax + Tmax).                                      dover = dL + u (Lmax + Tmax)
  * the curve c(over) is continuous with a slope within [0, 1], so an error of `over` passes at most unchanged, and a
    branch taken differently by the two costs nothing beyond it.  Its own roundings inside the knee: over + knee (u 2K),
    the square and the product by kq (2 u c, c <= K); a kq that is 1 / (4 knee) only to float32 leaves a step of at most
    u K at the knee's upper edge.  Together at most 7 u K.                                          dc = dover + 7 u K
  * g = fmaxf(slope c, range): the product's rounding u G; fmaxf passes errors unchanged.            dg = S dc + u G
  * the smoothing s' = g + al (s - g) is a convex combination of s and g, whichever of att and rel each side takes:
    if both take the same al, e' = al e_s + (1 - al) e_g; if they differ, s - g has opposite signs on the two sides
    and e' = e_g + th (e_s - e_g) with 0 <= th <= A again.  So injected errors do not grow; each step adds its own
    two roundings (s - g: u G; the fmaf: u G), which the recurrence keeps within 2 u G / (1 - A).
                                                                                    bound = dg + 2 u G / (1 - A)
Derived, not measured; the figures of every case: pytest -s.

The tests of the restatement need the library only for the coefficients (gab_dyn_poly); without the feature every test
here fails at that call or at the import, and every test of tests/test_dynamics_gpu.py.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits
from test_mix_host import EPS, fma32, mix_ramp

f32 = np.float32
UNIT = 20.0 * np.log10(2.0)                   # dB per log2 unit
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1, -256], np.float32)
THR, SLOPE, KNEE, KQ, ATT, REL, MAKEUP, RANGE = range(8)


@functools.lru_cache(maxsize=None)
def poly():
    """(c0..c6, d0..d6) as the library pins them."""
    from gpuaudiobench_amd import _capi
    pc, pd = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_float)()
    nc, nd = ctypes.c_int(0), ctypes.c_int(0)
    _capi.check(_capi.lib.gab_dyn_poly(ctypes.byref(pc), ctypes.byref(nc), ctypes.byref(pd), ctypes.byref(nd)))
    assert nc.value == 7 and nd.value == 7
    c, d = np.array([pc[k] for k in range(7)], np.float32), np.array([pd[k] for k in range(7)], np.float32)
    c.setflags(write=False)
    d.setflags(write=False)
    return c, d


def fmax32(a, b):
    """fmaxf: a NaN operand is ignored, -0 is below +0."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    with np.errstate(invalid="ignore"):
        r = np.where(a > b, a, np.where(b > a, b, np.where(np.signbit(a), b, a)))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, r)).astype(np.float32)


def fmin32(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    with np.errstate(invalid="ignore"):
        r = np.where(a < b, a, np.where(b < a, b, np.where(np.signbit(a), a, b)))
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, r)).astype(np.float32)


def horner32(c, x):
    r = np.full(np.shape(x), c[6], np.float32)
    for k in range(5, -1, -1):
        r = fma32(r, x, c[k])
    return r


def dyn_level_f32(a):
    """L of the contract for a detector value a >= 0 (float32, any shape)."""
    c, _ = poly()
    u = fmax32(a, f32(2.0 ** -96)).view(np.uint32)
    e = (u >> np.uint32(23)).astype(np.int32) - 127
    m = ((u & np.uint32(0x7fffff)) | np.uint32(0x3f800000)).view(np.float32)
    t = m - f32(1.0)
    L = e.astype(np.float32) + t * horner32(c, t)
    assert L.dtype == np.float32
    return L


def dyn_curve_f32(L, thr, slope, knee, kq, rng):
    over = L - thr
    ok = over + knee
    soft = (ok * ok) * kq
    c = np.where(over <= -knee, f32(0.0), np.where(over >= knee, over, soft)).astype(np.float32)
    g = fmax32(slope * c, rng)
    assert over.dtype == np.float32 and soft.dtype == np.float32 and g.dtype == np.float32
    return g


def dyn_gain_f32(s):
    """q * 2^floor: the linear gain of a smoothed gain s, before makeup."""
    _, d = poly()
    sc = fmin32(fmax32(s, f32(-126.0)), f32(0.0))
    nf = np.floor(sc)
    f = sc - nf
    q = horner32(d, f)
    scale = ((nf.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)
    return q * scale


def detector(k, link):
    """a [T][B]: |k| from 0 with NaN ignored, the maximum over each link group."""
    T, B = k.shape
    a = fmax32(f32(0.0), np.abs(k))
    return np.repeat(a.reshape(T // link, link, B).max(axis=1), link, axis=0)


def sample_params(cur, tgt, ramp, B):
    """[8][T][B] float32: the target, or on a ramp buffer fmaf(target - current, r[s], current)."""
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    if ramp is None:
        return np.broadcast_to(tgt.T[:, :, None], (8, tgt.shape[0], B))
    diff = (tgt - cur).T[:, :, None]                                  # float32: one rounding
    return fma32(diff, np.asarray(ramp, np.float32)[None, None, :], cur.T[:, :, None])


def _run(x, key, cur, tgt, ramp, s, link, wide):
    x = np.asarray(x, np.float32)
    T, B = x.shape
    k = x if key is None else np.asarray(key, np.float32)
    p = sample_params(cur, tgt, ramp, B)
    a = detector(k, link)
    with np.errstate(invalid="ignore", over="ignore"):
        if wide:
            p = p.astype(np.float64)
            L = np.log2(np.maximum(a.astype(np.float64), 2.0 ** -96))
            over = L - p[THR]
            c = np.where(over <= -p[KNEE], 0.0, np.where(over >= p[KNEE], over, (over + p[KNEE]) ** 2 * p[KQ]))
            g = np.maximum(p[SLOPE] * c, p[RANGE])
        else:
            g = dyn_curve_f32(dyn_level_f32(a), p[THR], p[SLOPE], p[KNEE], p[KQ], p[RANGE])
        S = np.empty((T, B), np.float64 if wide else np.float32)
        s = np.array(s, S.dtype)
        for n in range(B):
            gn = g[:, n]
            al = np.where(gn < s, p[ATT][:, n], p[REL][:, n])
            s = al * (s - gn) + gn if wide else fma32(al, s - gn, gn)
            S[:, n] = s
        if wide:
            y = x.astype(np.float64) * (np.exp2(np.clip(S, -126.0, 0.0)) * p[MAKEUP])
            gr = S.min(axis=1)
        else:
            y = x * (dyn_gain_f32(S) * p[MAKEUP])
            gr = np.full(T, np.inf, np.float32)
            for n in range(B):
                gr = fmin32(gr, S[:, n])
    return y, gr, s, S


def dyn_reference_f32(x, key, cur, tgt, ramp, s, link=1):
    """x, key [T][B] float32 (key may be None), cur / tgt [T][8] float32; ramp: the table [B] on a buffer with a pending
    ramp, else None; s [T]: the carried smoothed gain.  Returns (y [T][B], gr [T], s afterwards [T]), all float32."""
    y, gr, s, _ = _run(x, key, cur, tgt, ramp, s, link, False)
    assert y.dtype == np.float32 and gr.dtype == np.float32 and s.dtype == np.float32
    return y, gr, s


def dyn_reference_f64(x, key, cur, tgt, ramp, s, link=1):
    y, gr, s, _ = _run(x, key, cur, tgt, ramp, s, link, True)
    return y, gr, s


class Twin:
    """The plan's state machine on the host: current, target, a pending ramp, the smoothed gain; process() is
    dyn_reference_f32."""

    def __init__(self, T, B, link=1):
        self.T, self.B, self.link = T, B, link
        self.cur = np.tile(IDENTITY, (T, 1))
        self.tgt = self.cur.copy()
        self.pending = False
        self.s = np.zeros(T, np.float32)

    def set_params(self, p, ramp=True, first_track=0):
        n = p.shape[0]
        self.tgt[first_track:first_track + n] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + n] = p

    def reset(self):
        self.s = np.zeros(self.T, np.float32)
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x, key=None):
        y, gr, self.s = dyn_reference_f32(x, key, self.cur, self.tgt, mix_ramp(self.B) if self.pending else None, self.s,
                                          self.link)
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y, gr


def dyn_bound(Lmax, Tmax, K, S, G, A):
    """The bound on |s32 - s64| of the module's docstring, in log2 units."""
    dL = 2.0 ** -18 + EPS * Lmax
    dover = dL + EPS * (Lmax + Tmax)
    dc = dover + 7.0 * EPS * K
    dg = S * dc + EPS * G
    return dg + 2.0 * EPS * G / (1.0 - A)


def row(thr=0.0, slope=0.0, knee=0.0, att=0.0, rel=0.0, makeup=1.0, rng=-256.0):
    kq = 1.0 / (4.0 * knee) if knee > 0 else 0.0
    return np.array([thr, slope, knee, kq, att, rel, makeup, rng], np.float64).astype(np.float32)


def table(T, **kw):
    return np.tile(row(**kw), (T, 1))


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def dyn_mix(T, seed):
    """Parameter rows that differ on neighbouring tracks: hard and soft knees, compressors, limiters and tracks that are
    off, fast and slow ballistics, a floor that bites on some."""
    rng = np.random.RandomState(seed)
    p = np.zeros((T, 8), np.float32)
    for t in range(T):
        kind = (t + seed) % 5
        knee = (0.0, 0.5, 2.0, 0.0, 1.0)[kind]
        slope = (-0.75, -0.5, -1.0, 0.0, -0.9)[(t // 2 + seed) % 5]
        p[t] = row(thr=rng.uniform(-6.0, -1.0), slope=slope, knee=knee, att=(0.0, 0.5, 0.9, 0.99, 0.2)[(t + 2 * seed) % 5],
                   rel=(0.999, 0.9, 0.0, 0.99, 0.5)[(t // 3 + seed) % 5], makeup=rng.uniform(0.5, 2.0),
                   rng=(-256.0, -1.5, -0.25)[(t + seed) % 3])
    return p


def run_stream(xs, p, s=None, key=None, link=1):
    """Buffers xs [n][T][B] at steady parameters p; returns (ys, grs, S [T][n B])."""
    n, T, B = xs.shape
    s = np.zeros(T, np.float32) if s is None else s
    ys, grs, Ss = [], [], []
    for k in range(n):
        y, gr, s, S = _run(xs[k], None if key is None else key[k], p, p, None, s, link, False)
        ys.append(y), grs.append(gr), Ss.append(S)
    return np.stack(ys), np.stack(grs), np.concatenate(Ss, axis=1)


# ---- the two polynomials ------------------------------------------------------------------------------------------
def test_log2_polynomial_over_every_mantissa():
    """|t r(t) - log2(1 + t)| <= 2^-18 over all 2^23 mantissas, with the contract's float32 chain."""
    c, _ = poly()
    worst = 0.0
    for lo in range(0, 1 << 23, 1 << 21):
        m = (np.arange(lo, lo + (1 << 21), dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32)
        t = m - f32(1.0)
        got = (t * horner32(c, t)).astype(np.float64)
        worst = max(worst, float(np.abs(got - np.log2(m.astype(np.float64))).max()))
    print("log2: worst absolute error %.3g = 2^%.2f" % (worst, np.log2(worst)))
    assert worst <= 2.0 ** -18
    # and through dyn_level_f32, exponent and all: exact powers of two, the floor and an infinity
    a = np.array([1.0, 2.0, 0.5, 2.0 ** -96, 2.0 ** -120, 0.0, np.inf, 2.0 ** 127], np.float32)
    assert np.array_equal(dyn_level_f32(a), np.array([0, 1, -1, -96, -96, -96, 128, 127], np.float32))


def test_exp2_polynomial():
    """|q(f) / exp2(f) - 1| <= 2^-22 over 2^21 evenly spaced f, and d0 is exactly 1."""
    _, d = poly()
    assert d[0] == 1.0
    f = (np.arange(1 << 21, dtype=np.float64) / float(1 << 21)).astype(np.float32)
    q = horner32(d, f).astype(np.float64)
    worst = float(np.abs(q / np.exp2(f.astype(np.float64)) - 1.0).max())
    print("exp2: worst relative error %.3g = 2^%.2f" % (worst, np.log2(worst)))
    assert worst <= 2.0 ** -22
    # the gain stage around it: whole exponents are exact, the clamp holds
    s = np.array([0.0, -1.0, -2.0, -126.0, -300.0, 0.5], np.float32)
    assert np.array_equal(dyn_gain_f32(s), np.array([1.0, 0.5, 0.25, 2.0 ** -126, 2.0 ** -126, 1.0], np.float32))


def test_the_tool_fits_the_pinned_coefficients():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "dyn_poly.py"), "--check"], capture_output=True,
                       text=True, cwd=root, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- known answers ----------------------------------------------------------------------------------------------
def test_a_new_plans_table_is_the_identity():
    T, B = 4, 300
    x = (noise(T, B, 1).astype(np.float64) * np.exp(np.random.RandomState(2).uniform(-80, 80, (T, B)))).astype(np.float32)
    x[0, 5], x[1, 7], x[2, 0], x[3, 299] = np.inf, -np.inf, 0.0, -0.0
    p = np.tile(IDENTITY, (T, 1))
    for link in (1, 2, 4):
        y, gr, s = dyn_reference_f32(x, None, p, p, None, np.zeros(T, np.float32), link)
        assert np.array_equal(bits(y), bits(x))
        assert not s.any() and not gr.any()
    y, _, _ = dyn_reference_f32(x, None, p, p, mix_ramp(B), np.zeros(T, np.float32))
    assert np.array_equal(bits(y), bits(x))


def test_ratio_four_twelve_db_over_settles_at_nine_db():
    thr_db = -20.0
    p = table(1, thr=thr_db / UNIT, slope=1.0 / 4.0 - 1.0, att=0.9, rel=0.9)
    x = np.full((1, 600), 10.0 ** ((thr_db + 12.0) / 20.0), np.float32)
    y, gr, s = dyn_reference_f32(x, None, p, p, None, np.zeros(1, np.float32))
    assert abs(float(s[0]) * UNIT + 9.0) < 1e-4
    assert abs(20.0 * np.log10(float(y[0, -1]) / float(x[0, -1])) + 9.0) < 1e-4
    assert gr[0] == s[0]


def test_the_knee_is_continuous_with_a_continuous_first_difference():
    knee, h = 0.5, 2.0 ** -10
    p = row(thr=0.0, slope=-1.0, knee=knee)
    for edge, slope_outside in ((-knee, 0.0), (knee, 1.0)):
        L = (edge + h * np.arange(-4, 5)).astype(np.float32)           # exact: multiples of 2^-10
        c = -dyn_curve_f32(L, p[THR], p[SLOPE], p[KNEE], p[KQ], p[RANGE]).astype(np.float64)
        want = np.where(L <= -knee, 0.0, np.where(L >= knee, L, (L.astype(np.float64) + knee) ** 2 / (4 * knee)))
        assert np.abs(c - want).max() <= 4 * EPS * knee               # the curve itself
        d = np.diff(c) / h
        # across the edge the first difference moves by the parabola's curvature, h / (2 knee) per step, and no more
        assert np.abs(np.diff(d)).max() <= 1.01 * h / (2 * knee) + 16 * EPS / h
        outside = d[:3] if slope_outside == 0.0 else d[-3:]
        assert np.abs(outside - slope_outside).max() <= 16 * EPS / h


def test_a_limiter_holds_a_settled_sines_peak_to_the_threshold():
    thr = -1.0                                                         # 0.5 linear
    p = table(1, thr=thr, slope=-1.0, att=0.0, rel=0.9999)
    n = np.arange(4800)
    x = (0.9 * np.sin(2 * np.pi * 1000.0 * n / 48000.0)).astype(np.float32)[None, :]
    y, gr, s = dyn_reference_f32(x, None, p, p, None, np.zeros(1, np.float32))
    peak = float(np.abs(y[0, 2400:]).max())
    assert abs(peak / 0.5 - 1.0) < 1e-5
    assert float(np.abs(y).max()) <= 0.5 * (1 + 1e-5)                  # instant attack: never above, from the first sample


@pytest.mark.parametrize("which", ["attack", "release"])
def test_time_constants(which):
    """After ms fs / 1000 samples the reduction has covered 1 - 1/e of its way."""
    from gpuaudiobench_amd import dynamics_params
    ms, fs = 2.0, 48000.0
    N = int(ms * fs / 1000.0)
    p = dynamics_params(-12.0, 4.0, 0.0, ms, ms, fs=fs)[None, :]
    loud, quiet = np.full((1, N), 1.0, np.float32), np.full((1, N), 1e-3, np.float32)
    goal = float(p[0, SLOPE]) * (0.0 - float(p[0, THR]))               # the settled reduction of the loud level
    if which == "attack":
        _, _, s = dyn_reference_f32(loud, None, p, p, None, np.zeros(1, np.float32))
        covered = float(s[0]) / goal
    else:
        _, _, s = dyn_reference_f32(quiet, None, p, p, None, np.full(1, goal, np.float32))
        covered = 1.0 - float(s[0]) / goal
    assert abs(covered - (1.0 - np.exp(-1.0))) < 1e-4


def test_range_floors_the_reduction():
    p = table(1, thr=-10.0, slope=-1.0, att=0.5, rel=0.5, rng=-1.0)
    x = np.full((1, 200), 1.0, np.float32)
    y, gr, s = dyn_reference_f32(x, None, p, p, None, np.zeros(1, np.float32))
    assert s[0] == -1.0 and gr[0] == -1.0 and y[0, -1] == 0.5
    p[0, RANGE] = -256.0
    _, _, s = dyn_reference_f32(x, None, p, p, None, np.zeros(1, np.float32))
    assert abs(float(s[0]) + 10.0) < 1e-5


def test_a_key_ducks_a_track_below_its_threshold():
    p = table(2, thr=-2.0, slope=-0.5, att=0.5, rel=0.5, makeup=1.5)
    x = np.full((2, 100), 0.125, np.float32)                           # L = -3: below the threshold
    key = np.stack([np.full(100, 1.0, np.float32), np.full(100, 0.125, np.float32)])
    y, _, s = dyn_reference_f32(x, None, p, p, None, np.zeros(2, np.float32))
    assert not s.any() and np.array_equal(y, x * f32(1.5))
    y, gr, s = dyn_reference_f32(x, key, p, p, None, np.zeros(2, np.float32))
    assert abs(float(s[0]) + 1.0) < 1e-5 and s[1] == 0.0             # over = 2 units, slope -0.5
    assert abs(float(y[0, -1]) / (0.125 * 1.5) - 0.5) < 1e-5 and y[1, -1] == f32(0.125) * f32(1.5)


def test_linked_tracks_share_the_louder_detector_and_keep_their_parameters():
    p = np.stack([row(thr=-2.0, slope=-0.5, att=0.5, rel=0.5), row(thr=-2.0, slope=-0.75, att=0.5, rel=0.5),
                  row(thr=-2.0, slope=-0.5, att=0.5, rel=0.5), row(thr=-2.0, slope=-0.75, att=0.5, rel=0.5)])
    x = np.stack([np.full(100, 0.125, np.float32), np.full(100, 1.0, np.float32),
                  np.full(100, 0.125, np.float32), np.full(100, 0.0625, np.float32)])
    _, _, s = dyn_reference_f32(x, None, p, p, None, np.zeros(4, np.float32), link=2)
    assert abs(float(s[0]) + 1.0) < 1e-5 and abs(float(s[1]) + 1.5) < 1e-5 and s[2] == 0.0 and s[3] == 0.0
    _, _, s = dyn_reference_f32(x, None, p, p, None, np.zeros(4, np.float32), link=1)
    assert s[0] == 0.0 and abs(float(s[1]) + 1.5) < 1e-5


def test_nonfinite_samples_reach_the_output_and_nothing_else():
    T, B = 2, 64
    p = table(T, thr=-4.0, slope=-0.5, att=0.5, rel=0.9)
    x = noise(T, B, 3)
    x[0, 10], x[0, 20], x[1, 30] = np.nan, np.inf, -np.inf
    y, gr, s, S = _run(x, None, p, p, None, np.zeros(T, np.float32), 1, False)
    assert np.isfinite(S).all() and np.isfinite(gr).all()
    assert np.isnan(y[0, 10]) and y[0, 20] == np.inf and y[1, 30] == -np.inf
    assert np.isfinite(np.delete(y[0], [10, 20])).all()
    a = detector(x, 1)
    assert a[0, 10] == 0.0 and dyn_level_f32(a)[0, 10] == -96.0 and dyn_level_f32(a)[0, 20] == 128.0
    # the NaN reads as silence: the stream's gains are those of the same block with a zero in its place
    x0 = x.copy()
    x0[0, 10] = 0.0
    assert np.array_equal(bits(_run(x0, None, p, p, None, np.zeros(T, np.float32), 1, False)[3]), bits(S))
    # in the key they never reach the output
    y, _, _, S = _run(noise(T, B, 4), x, p, p, None, np.zeros(T, np.float32), 2, False)
    assert np.isfinite(y).all() and np.isfinite(S).all()


def test_dynamics_params():
    from gpuaudiobench_amd import dynamics_params
    r = dynamics_params(-18.0, 4.0, 6.0, 5.0, 100.0, makeup_db=6.0, range_db=-24.0, fs=48000.0)
    assert r.shape == (8,) and r.dtype == np.float32
    want = [-18.0 / UNIT, -0.75, 3.0 / UNIT, UNIT / 12.0, np.exp(-1.0 / 240.0), np.exp(-1.0 / 4800.0),
            10.0 ** 0.3, -24.0 / UNIT]
    assert np.array_equal(r, np.array(want, np.float64).astype(np.float32))
    r = dynamics_params(0.0, np.inf, 0.0, 0.0, 0.0)
    assert np.array_equal(r, np.array([0, -1, 0, 0, 0, 0, 1, -256], np.float32))
    t = dynamics_params([-10.0, -20.0, -30.0], 2.0, [0.0, 3.0, 6.0], 1.0, 50.0)
    assert t.shape == (3, 8) and t[0, KQ] == 0.0 and (t[:, SLOPE] == -0.5).all()
    assert dynamics_params(0.0, 2.0, 0.0, 1e9, 1e9)[ATT] == f32(1.0 - 2.0 ** -20)
    for bad in ((0.0, 0.5, 0.0, 1.0, 1.0), (0.0, 2.0, -1.0, 1.0, 1.0), (0.0, 2.0, 0.0, -1.0, 1.0)):
        with pytest.raises(ValueError):
            dynamics_params(*bad)


# ---- float32 against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("knee", ["hard", "soft"])
@pytest.mark.parametrize("link", [1, 2])
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("ramp", [False, True])
def test_float32_is_within_its_bound_of_float64(knee, link, keyed, ramp):
    T, B, n = 16, 64, 10
    A, K, S, G, Tmax = 0.999, (2.0 if knee == "soft" else 0.0), 1.0, 8.0, 8.0
    rng = np.random.RandomState(7 + link + 2 * keyed)

    def rows():
        p = np.zeros((T, 8), np.float32)
        for t in range(T):
            p[t] = row(thr=rng.uniform(-Tmax, 0.0), slope=-rng.uniform(0.3, S), knee=rng.uniform(0.25, K) if K else 0.0,
                       att=rng.uniform(0.0, A), rel=rng.uniform(0.9, A), makeup=rng.uniform(0.5, 2.0),
                       rng=-rng.uniform(2.0, G))
        p[0, ATT], p[1, REL], p[2, SLOPE], p[3, RANGE] = A, A, -S, -G
        return p

    tables = [rows(), rows()]
    cur = tgt = tables[0]
    scale = np.exp2(rng.uniform(-10.0, 2.0, (T, 1)))
    s32, s64 = np.zeros(T, np.float32), np.zeros(T, np.float64)
    worst, Lmax = 0.0, 0.0
    for k in range(n):
        x = (noise(T, B, 300 + k) * scale * (1.0 if k % 4 else 8.0)).astype(np.float32)
        key = (noise(T, B, 400 + k) * scale).astype(np.float32) if keyed else None
        r = None
        if ramp and k % 3 == 1:
            tgt = tables[(k // 3 + 1) % 2]                             # a new target: the ramp runs from the old one
            r = mix_ramp(B)
        det = np.abs(x if key is None else key).astype(np.float64)
        Lmax = max(Lmax, float(np.abs(np.log2(np.maximum(det, 2.0 ** -96))).max()))
        _, _, s32, S32 = _run(x, key, cur, tgt, r, s32, link, False)
        _, _, s64, S64 = _run(x, key, cur, tgt, r, s64, link, True)
        worst = max(worst, float(np.abs(S32.astype(np.float64) - S64).max()))
        if r is not None:
            cur = tgt
    assert Lmax <= 32.0                                                # the levels this bound is stated for
    bound = dyn_bound(32.0, Tmax, K, S, G, A)
    print("%s knee, link %d, %s, %s: |s32 - s64| %.3g units, bound %.3g units = %.4f dB (err / bound %.3g)"
          % (knee, link, "keyed" if keyed else "own input", "ramps" if ramp else "steady", worst, bound, bound * UNIT,
             worst / bound))
    assert bound * UNIT <= 0.01                                        # the bound itself means something
    assert worst <= bound


# ---- the library without a GPU --------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 1), (-1, 512, 1), (4, 0, 1), (4, -5, 1), (4, 512, 0), (4, 512, -2), (4, 512, 3), (6, 512, 4),
                 (128, 512, 128), (64, 512, 48), (3, 512, 2)):
        assert lib.gab_dyn_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_dyn_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_dyn_create(None, 4, 512, 1) == bad
    assert b"gab_dyn_create" in lib.gab_last_error() and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_dyn_process(None, None, None, None, None, None), b"gab_dyn_process"),
                       (lambda: lib.gab_dyn_process_batch(None, None, None, None, None, 1, None), b"gab_dyn_process_batch"),
                       (lambda: lib.gab_dyn_set_params(None, None, 1, None), b"gab_dyn_set_params"),
                       (lambda: lib.gab_dyn_set_params_tracks(None, None, 0, 1, 1, None), b"gab_dyn_set_params_tracks"),
                       (lambda: lib.gab_dyn_params(None, None, None, None), b"gab_dyn_params"),
                       (lambda: lib.gab_dyn_state(None, None, None), b"gab_dyn_state"),
                       (lambda: lib.gab_dyn_poly(None, None, None, None), b"gab_dyn_poly"),
                       (lambda: lib.gab_dyn_reset(None, None), b"gab_dyn_reset"),
                       (lambda: lib.gab_dyn_destroy(None), b"gab_dyn_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_dynamics_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_dyn_create(C.byref(h), 4, 512, 2)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_dyn_create" in text


def test_dynamics_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "DynamicsPlan" in g.__all__ and callable(g.DynamicsPlan) and "dynamics_params" in g.__all__
    for name in ("set_params", "reset", "process", "process_batch", "params", "state", "prepare", "launch", "close"):
        assert hasattr(g.DynamicsPlan, name), name
    assert len(g.DynamicsPlan.FIELDS) == 8
