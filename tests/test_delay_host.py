"""The delay plan (gab_delay_*) without a GPU: the restatement the GPU tests compare against, held without trusting it.

    Line                 a plan's lines on the host: per track the last max_delay + 3 values that entered the line.
    delay_reference_f32  the contract of include/gab_c_api.h in numpy, vectorised over tracks, one sample at a time:
                         every operation a float32 operation rounded once, fma32 (tests/test_mix_host.py) where the
                         contract says fmaf.  What delay_kernel must equal bit for bit.
    delay_reference_f64  its twin: the same float32 parameters per sample (delay, i, fr, feedback, wet, dry are the
                         control path and are the contract's), the signal path (weights, tap, w, y) in float64.

The a-priori bound of float32 against float64 (delay_bound), u = 2^-24, W >= |w|, F >= |feedback|, L the sum of the
absolute interpolation weights (1 for linear, whose weights are 1 - fr and fr; at most 1.25 for third-order Lagrange on
[0, 1], reached at fr = 0.5: 1/16 + 9/16 + 9/16 + 1/16):
  * the tap from exact inputs.  Linear: b - a is one rounding, at most u (|a| + |b|) <= 2 u W, the fmaf another, u |v|
    <= u W: 3 u W.  Lagrange: fm1, fm2, fp1 one rounding each, three products per weight, the constant 1/6 one more:
    each weight to 7 u relative; the product and the three fmaf of the sum one rounding each of a partial sum that is at
    most L W: (7 + 4) u L W = 11 u L W.  k = 3 or 11, in units of u L W.
  * into the line: w = fmaf(feedback, v, x) is one rounding, u W, on top of F times the tap's error:
    fresh = (F k L + 1) u W.
  * the error E of w obeys E[n] <= F L max(E before n) + fresh, so E <= fresh / (1 - F L): the amplification of the
    feedback loop, 1 / (1 - F) for linear.  It needs F L < 1: the Lagrange cases use |feedback| <= 0.7.
  * the output: y = fmaf(wet, v, dry x): |wet| (L E + k u L W) from the tap, u |dry x| and u |y| from the two roundings.
Derived, not measured; the figures of every case: pytest -s.

The tests of the restatement need nothing of the library and pass on any commit; what fails without the feature is the
argument checks, the runtime-mode refusal and the export test here, and every test of tests/test_delay_gpu.py.
"""
import ctypes

import numpy as np
import pytest

from plan_helpers import bits
from test_mix_host import EPS, fma32, mix_ramp

INTERPS = ("linear", "lagrange3")
C6 = np.float32(1.0 / 6.0)
f32 = np.float32


def min_delay(interp):
    return 2 if interp == "lagrange3" else 1


def capacity(bufsize, max_delay):
    cap = 1
    while cap < max_delay + 3 + bufsize:
        cap *= 2
    return cap


class Line:
    """hist [T][max_delay + 3]: the values that entered the line, the newest last; zero before the first sample."""

    def __init__(self, tracks, max_delay, dtype=np.float32):
        self.max_delay = int(max_delay)
        self.hist = np.zeros((tracks, self.max_delay + 3), dtype)
        self.count = 0                       # samples so far

    def rows(self, a, b):
        out = Line(b - a, self.max_delay, self.hist.dtype)
        out.hist[:] = self.hist[a:b]
        out.count = self.count
        return out


def delay_params_f32(cur, tgt, r, interp, max_delay):
    """The four parameters of one sample, [T] each: the ramp (r a float32, or None on a buffer without one), then the
    clamp on the delay alone."""
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    if r is None:
        d, fb, wet, dry = (tgt[:, c] for c in range(4))
    else:
        diff = tgt - cur                                     # float32: one rounding
        d, fb, wet, dry = (fma32(diff[:, c], f32(r), cur[:, c]) for c in range(4))
    d = np.minimum(np.maximum(d, f32(min_delay(interp))), f32(max_delay))
    return d.astype(np.float32), fb, wet, dry


def split(d):
    fl = np.floor(d)
    fr = d - fl                                              # exact
    assert fr.dtype == np.float32
    return fl.astype(np.int64), fr


def lagrange_weights_f32(fr):
    fm1, fm2, fp1 = fr - f32(1.0), fr - f32(2.0), fr + f32(1.0)
    hm = ((fr * fm1) * fm2) * (-C6)
    h0 = ((fp1 * fm1) * fm2) * f32(0.5)
    h1 = ((fp1 * fr) * fm2) * f32(-0.5)
    h2 = ((fp1 * fr) * fm1) * C6
    for h in (hm, h0, h1, h2):
        assert h.dtype == np.float32
    return hm, h0, h1, h2


def lagrange_weights_f64(fr):
    fr = fr.astype(np.float64)
    return (-fr * (fr - 1) * (fr - 2) / 6.0, (fr + 1) * (fr - 1) * (fr - 2) / 2.0, -(fr + 1) * fr * (fr - 2) / 2.0,
            (fr + 1) * fr * (fr - 1) / 6.0)


def _run(x, cur, tgt, ramp, line, interp, wide):
    x = np.asarray(x, np.float32)
    T, B = x.shape
    H = line.hist.shape[1]
    dt = np.float64 if wide else np.float32
    assert line.hist.dtype == dt
    buf = np.concatenate([line.hist, np.zeros((T, B), dt)], axis=1)
    y = np.zeros((T, B), dt)
    rows = np.arange(T)
    steady = None if ramp is not None else delay_params_f32(cur, tgt, None, interp, line.max_delay)
    for s in range(B):
        d, fb, wet, dry = steady if ramp is None else delay_params_f32(cur, tgt, ramp[s], interp, line.max_delay)
        i, fr = split(d)
        assert (i >= min_delay(interp)).all() and (i <= line.max_delay).all()
        k = H + s - i
        a, b = buf[rows, k], buf[rows, k - 1]
        xs = x[:, s]
        if wide:
            if interp == "linear":
                v = a + fr.astype(np.float64) * (b - a)
            else:
                hm, h0, h1, h2 = lagrange_weights_f64(fr)
                v = hm * buf[rows, k + 1] + h0 * a + h1 * b + h2 * buf[rows, k - 2]
            buf[:, H + s] = fb.astype(np.float64) * v + xs
            y[:, s] = wet.astype(np.float64) * v + dry.astype(np.float64) * xs
        else:
            if interp == "linear":
                v = fma32(fr, b - a, a)
            else:
                hm, h0, h1, h2 = lagrange_weights_f32(fr)
                v = hm * buf[rows, k + 1]
                v = fma32(h1, b, v)
                v = fma32(h2, buf[rows, k - 2], v)
                v = fma32(h0, a, v)
            buf[:, H + s] = fma32(fb, v, xs)
            y[:, s] = fma32(wet, v, dry * xs)
    line.hist = np.ascontiguousarray(buf[:, B:])
    line.count += B
    return y


def delay_reference_f32(x, cur, tgt, ramp, line, interp):
    """x [T][B] float32, cur / tgt [T][4] float32; ramp: the table [B] on a buffer with a pending ramp, else None;
    line: a float32 Line, moved on by B samples.  Returns y [T][B] float32."""
    y = _run(x, cur, tgt, ramp, line, interp, False)
    assert y.dtype == np.float32 and line.hist.dtype == np.float32
    return y


def delay_reference_f64(x, cur, tgt, ramp, line, interp):
    return _run(x, cur, tgt, ramp, line, interp, True)


class Twin:
    """The plan's state machine on the host: current, target, a pending ramp, the lines; process() is
    delay_reference_f32."""

    def __init__(self, T, B, max_delay, interp):
        self.T, self.B, self.M, self.interp = T, B, max_delay, interp
        self.cur = table(T, min_delay(interp), 0.0, 0.0, 1.0)
        self.tgt = self.cur.copy()
        self.pending = False
        self.line = Line(T, max_delay)

    def set_params(self, p, ramp=True, first_track=0):
        n = p.shape[0]
        self.tgt[first_track:first_track + n] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + n] = p

    def reset(self):
        self.line = Line(self.T, self.M)
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x):
        y = delay_reference_f32(x, self.cur, self.tgt, mix_ramp(self.B) if self.pending else None, self.line, self.interp)
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y


def delay_bound(interp, F, W, wet=1.0, out_peak=0.0):
    """(bound on |w32 - w64|, bound on |y32 - y64|): the derivation in the module's docstring."""
    lam, k = (1.0, 3.0) if interp == "linear" else (1.25, 11.0)
    assert F * lam < 1.0
    fresh = (F * k * lam + 1.0) * EPS * W
    e_w = fresh / (1.0 - F * lam)
    e_y = wet * (lam * e_w + k * EPS * lam * W) + 2.0 * EPS * out_peak
    return e_w, e_y


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def table(T, delay, fb=0.0, wet=1.0, dry=0.0):
    p = np.zeros((T, 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = delay, fb, wet, dry
    return p


def delay_mix(T, B, max_delay, interp, seed):
    """Parameter rows that differ on neighbouring tracks: delays of at least a buffer, between a wave and a buffer, below
    a wave, exactly min_delay with feedback (the serial case), fractional and integer, feedback of both signs and 0."""
    rng = np.random.RandomState(seed)
    lo = min_delay(interp)
    p = np.zeros((T, 4), np.float32)
    for t in range(T):
        kind = (t + seed) % 6
        if kind == 0:
            d = rng.uniform(min(B, max_delay), max_delay)
        elif kind == 1:
            d = rng.uniform(min(64, max_delay), min(max(B, 64), max_delay))
        elif kind == 2:
            d = rng.uniform(lo, min(64, max_delay))
        elif kind == 3:
            d = lo
        elif kind == 4:
            d = float(rng.randint(lo, max_delay + 1))
        else:
            d = rng.uniform(lo, max_delay)
        fb = (0.0, 0.6, -0.7, 0.5, -0.3, 0.0)[(t // 2 + seed) % 6] if kind != 3 else (0.65 if t % 2 else -0.65)
        p[t] = (d, fb, rng.uniform(-1, 1), rng.uniform(-1, 1))
    p[:, 0] = np.minimum(np.maximum(p[:, 0], f32(lo)), f32(max_delay))
    return p


# ---- the restatement, held by what a delay line must do ----------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("D,B", [(2, 7), (5, 16), (16, 16), (37, 10), (100, 64)])
def test_integer_delays_are_exact_shifts(interp, D, B):
    T, n = 3, 6
    x = noise(T, n * B, D + B)
    line = Line(T, max(D, 2))
    p = table(T, D)
    y = np.concatenate([delay_reference_f32(x[:, k * B:(k + 1) * B], p, p, None, line, interp) for k in range(n)], axis=1)
    assert not y[:, :D].any()
    assert np.array_equal(bits(y[:, D:]), bits(x[:, :-D]))


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("D,B", [(2, 5), (7, 16), (24, 8)])
def test_known_answer_echo(interp, D, B):
    n = 12
    x = np.zeros((1, n * B), np.float32)
    x[0, 0] = 1.0
    line = Line(1, D)
    p = table(1, D, fb=0.5)
    y = np.concatenate([delay_reference_f32(x[:, k * B:(k + 1) * B], p, p, None, line, interp) for k in range(n)], axis=1)[0]
    want = np.zeros(n * B, np.float32)
    for k in range(1, (n * B - 1) // D + 1):
        want[k * D] = 0.5 ** (k - 1)
    assert np.array_equal(y, want)


@pytest.mark.parametrize("delay", [1.25, 7.3, 20.999, 33.5])
def test_linear_reproduces_a_straight_line(delay):
    """x[n] = alpha n + beta, rounded to float32 (u |x| each).  With feedback 0 the line holds x itself (w = 0 v + x),
    and y = v: a convex combination of two inputs (their roundings: u X) computed with the tap's 3 u X: 4 u X."""
    T, B, n = 1, 32, 4
    d = f32(delay)
    idx = np.arange(n * B, dtype=np.float64)
    alpha, beta = 0.37, -11.0
    x = (alpha * idx + beta).astype(np.float32)[None, :]
    line = Line(T, 40)
    p = table(T, d)
    y = np.concatenate([delay_reference_f32(x[:, k * B:(k + 1) * B], p, p, None, line, "linear") for k in range(n)], axis=1)[0]
    first = int(np.ceil(float(d))) + 1
    truth = alpha * (idx - float(d)) + beta
    err = np.abs(y.astype(np.float64) - truth)[first:]
    bound = 4 * EPS * np.abs(x).max()
    print("linear, delay %.3f: worst err / bound %.3g" % (delay, err.max() / bound))
    assert err.max() <= bound


@pytest.mark.parametrize("delay", [2.0, 2.25, 7.3, 20.999, 33.5])
def test_lagrange3_reproduces_a_cubic(delay):
    """x a cubic in n, rounded to float32.  The inputs' roundings reach the output through the weights (L u X) and the
    tap adds its 11 u L X: 12 L u X, L = 1.25."""
    T, B, n = 1, 32, 4
    d = f32(delay)
    idx = np.arange(n * B, dtype=np.float64)

    def cubic(t):
        t = t / 64.0
        return 0.8 * t ** 3 - 1.7 * t ** 2 + 0.4 * t + 0.3

    x = cubic(idx).astype(np.float32)[None, :]
    line = Line(T, 40)
    p = table(T, d)
    y = np.concatenate([delay_reference_f32(x[:, k * B:(k + 1) * B], p, p, None, line, "lagrange3") for k in range(n)], axis=1)[0]
    first = int(np.ceil(float(d))) + 3
    err = np.abs(y.astype(np.float64) - cubic(idx - float(d)))[first:]
    bound = 12 * 1.25 * EPS * np.abs(x).max()
    print("lagrange3, delay %.3f: worst err / bound %.3g" % (delay, err.max() / bound))
    assert err.max() <= bound
    # and linear does not: the cubic test bites
    line = Line(T, 40)
    yl = np.concatenate([delay_reference_f32(x[:, k * B:(k + 1) * B], p, p, None, line, "linear") for k in range(n)], axis=1)[0]
    if 0.2 < float(d) - np.floor(float(d)) < 0.8:
        assert np.abs(yl.astype(np.float64) - cubic(idx - float(d)))[first:].max() > bound


def test_lagrange_weights():
    fr = np.linspace(0.0, 1.0, 4097)[:-1].astype(np.float32)
    h32 = lagrange_weights_f32(fr)
    h64 = lagrange_weights_f64(fr)
    assert np.abs(sum(h64) - 1.0).max() < 1e-15
    lam = sum(np.abs(h) for h in h64)
    assert lam.max() <= 1.25 and lam[2048] == 1.25
    for a, b in zip(h32, h64):
        assert (np.abs(a.astype(np.float64) - b) <= 7 * EPS * np.abs(b)).all()
    # fr == 0: the weights are (0, 1, 0, 0), h0 exactly one
    z = lagrange_weights_f32(np.zeros(1, np.float32))
    assert z[1][0] == 1.0 and z[0][0] == 0.0 and z[2][0] == 0.0 and z[3][0] == 0.0


@pytest.mark.parametrize("interp,F", [("linear", 0.9), ("linear", 0.5), ("lagrange3", 0.7), ("lagrange3", 0.3)])
@pytest.mark.parametrize("ramp", [False, True])
def test_float32_is_within_its_bound_of_float64(interp, F, ramp):
    T, B, n, M = 24, 64, 12, 300
    rng = np.random.RandomState(int(F * 10) + len(interp))
    lo = min_delay(interp)
    cur, tgt = table(T, 1), table(T, 1)
    for p in (cur, tgt):
        p[:, 0] = rng.uniform(lo, M, T).astype(np.float32)
        p[::3, 0] = rng.uniform(lo, 8, len(p[::3]))
        p[:, 1] = rng.uniform(-F, F, T)
        p[0, 1], p[1, 1] = F, -F
        p[:, 2] = rng.uniform(-1, 1, T)
        p[:, 3] = rng.uniform(-1, 1, T)
    l32, l64 = Line(T, M), Line(T, M, np.float64)
    W = Y = 0.0
    errs = []
    for k in range(n):
        x = noise(T, B, 500 + k)
        r = None
        if ramp and k % 3 == 1:
            cur, tgt = tgt, cur                                  # a new target: the ramp runs from the old one
            r = mix_ramp(B)
        y32 = delay_reference_f32(x, cur, tgt, r, l32, interp)
        y64 = delay_reference_f64(x, cur, tgt, r, l64, interp)
        W = max(W, float(np.abs(l64.hist).max()))
        Y = max(Y, float(np.abs(y64).max()))
        errs.append((float(np.abs(l32.hist.astype(np.float64) - l64.hist).max()),
                     float(np.abs(y32.astype(np.float64) - y64).max())))
    e_w, e_y = delay_bound(interp, F, 1.01 * W, wet=1.0, out_peak=1.01 * Y)
    worst_w, worst_y = max(e[0] for e in errs), max(e[1] for e in errs)
    print("%s, |feedback| <= %.1f, %s: |w| <= %.3g; line err / bound %.3g, output err / bound %.3g, bound / peak %.3g"
          % (interp, F, "ramps" if ramp else "steady", W, worst_w / e_w, worst_y / e_y, e_y / Y))
    assert worst_w <= e_w and worst_y <= e_y
    assert e_w <= 0.01 * W and e_y <= 1e-4 * Y          # far below signal level


# ---- the clamp --------------------------------------------------------------------------------------------------
# The contract clamps the ramped delay because a ramp's value could in principle leave [current, target] by a rounding.
# For the tables a plan can hold it cannot leave [min_delay, max_delay] downwards, and the search below holds that:
# current and target are float32 in [min_delay, 2^20], so current is a multiple of its own ulp (at most 2^-3) and so is
# the integer min_delay; min_delay - current is then a multiple of that ulp of smaller magnitude than current, hence a
# float32.  Rounding is monotone, so fl(target - current) >= min_delay - current, and with 0 < r <= 1 the exact value
# current + fl(target - current) r is at least min_delay; the fmaf's one rounding cannot take it below a float32.
# No admissible (current, target) pair therefore has an unclamped value below min_delay: the pair the clamp is shown on
# is one that set_params refuses (a current below min_delay), which only the restatement can be handed.
def _unclamped(cur, tgt, r):
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    return fma32(tgt - cur, f32(r), cur)


@pytest.mark.parametrize("interp", INTERPS)
def test_the_clamp(interp):
    lo = min_delay(interp)
    for B in (1, 3, 64, 100, 512):
        r = mix_ramp(B)
        for s in range(B):
            d, _, _, _ = delay_params_f32(table(1, 5.3), table(1, lo), r[s], interp, 1000)
            i, fr = split(d)
            assert i[0] >= lo and d[0] >= lo
        assert d[0] == lo
    # no admissible pair undershoots or overshoots: random pairs, pairs an ulp from the ends, every table value of r
    rng = np.random.RandomState(4)
    n, M = 20000, 2 ** 20
    cur = np.exp(rng.uniform(np.log(lo), np.log(M), n)).astype(np.float32)
    tgt = np.exp(rng.uniform(np.log(lo), np.log(M), n)).astype(np.float32)
    tgt[:5000] = np.nextafter(f32(lo), f32(M))
    tgt[5000:8000] = lo
    cur[8000:10000] = np.nextafter(f32(lo), f32(M))
    tgt[10000:12000] = M
    cur, tgt = np.clip(cur, lo, M), np.clip(tgt, lo, M)
    for r in np.concatenate([mix_ramp(512)[[0, 1, 255, 510, 511]], mix_ramp(100)[[0, 50, 98, 99]], mix_ramp(3)]):
        v = _unclamped(cur, tgt, r)
        assert (v >= lo).all() and (v <= M).all()
    # the clamp itself, on a pair no plan can hold: current 0.25 is below min_delay
    cur, tgt = f32(0.25), f32(lo)
    assert _unclamped(cur, tgt, mix_ramp(16)[3]) < lo
    B = 16
    for s in range(B):
        d, _, _, _ = delay_params_f32(table(1, cur), table(1, tgt), mix_ramp(B)[s], interp, 16)
        assert d[0] == lo
    y = delay_reference_f32(noise(1, B, 3), table(1, cur, fb=0.5), table(1, tgt, fb=0.5), mix_ramp(B), Line(1, 16), interp)
    assert np.isfinite(y).all()
    d, _, _, _ = delay_params_f32(table(1, 2.0), table(1, 40.0), f32(1.0), interp, 16)
    assert d[0] == 16.0


def test_a_ramp_is_monotone():
    """What lets a kernel take the smallest integer delay of a buffer from its two ends."""
    rng = np.random.RandomState(9)
    for B in (7, 100, 512):
        r = mix_ramp(B)
        cur, tgt = table(200, rng.uniform(1, 5000, 200)), table(200, rng.uniform(1, 5000, 200))
        d = np.stack([delay_params_f32(cur, tgt, r[s], "linear", 4096)[0] for s in range(B)], axis=1)
        up = tgt[:, 0] >= cur[:, 0]
        assert (np.diff(d[up], axis=1) >= 0).all() and (np.diff(d[~up], axis=1) <= 0).all()


# ---- the library without a GPU --------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 100, 0), (-1, 512, 100, 0), (4, 0, 100, 0), (4, -5, 100, 0), (4, 512, 0, 0), (4, 512, 1, 1),
                 (4, 512, 2 ** 20 + 1, 0), (4, 512, -7, 1), (4, 512, 100, 2), (4, 512, 100, -1)):
        assert lib.gab_delay_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_delay_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_delay_create(None, 4, 512, 100, 0) == bad
    assert b"gab_delay_create" in lib.gab_last_error() and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_delay_process(None, None, None, None), b"gab_delay_process"),
                       (lambda: lib.gab_delay_process_batch(None, None, None, 1, None), b"gab_delay_process_batch"),
                       (lambda: lib.gab_delay_set_params(None, None, 1, None), b"gab_delay_set_params"),
                       (lambda: lib.gab_delay_set_params_tracks(None, None, 0, 1, 1, None), b"gab_delay_set_params_tracks"),
                       (lambda: lib.gab_delay_params(None, None, None, None), b"gab_delay_params"),
                       (lambda: lib.gab_delay_line(None, None, None, None), b"gab_delay_line"),
                       (lambda: lib.gab_delay_reset(None, None), b"gab_delay_reset"),
                       (lambda: lib.gab_delay_destroy(None), b"gab_delay_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_delay_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_delay_create(C.byref(h), 4, 512, 100, 0)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_delay_create" in text


def test_delay_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "DelayPlan" in g.__all__ and callable(g.DelayPlan)
    for name in ("set_params", "reset", "process", "process_batch", "params", "line", "prepare", "launch", "close"):
        assert hasattr(g.DelayPlan, name), name
    assert g._capi.DELAY_LINEAR == 0 and g._capi.DELAY_LAGRANGE3 == 1
    with pytest.raises(ValueError):
        g.DelayPlan(4, 64, 100, interp="cubic")
