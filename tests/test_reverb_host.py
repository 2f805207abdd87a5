"""The reverb plan (gab_reverb_*) without a GPU: the restatement the GPU tests compare against, held without trusting it.

    reverb_reference_f32  the contract of include/gab_c_api.h in numpy, vectorised over tracks and lines: every
                          operation a float32 operation rounded once, fma32 (tests/test_mix_host.py) where the contract
                          says fmaf.  The low-pass (step 3) is a Python loop over samples; the steps around it are taken
                          32 samples at a time, which the contract's smallest delay allows and which changes no bit.
                          What reverb_kernel must equal bit for bit.
    reverb_reference_f64  its twin: the same float32 parameters per sample (they are the control path and the
                          contract's), the network in float64.
    Twin                  the plan's state machine on the host: current, target, a pending ramp, delays, the lines'
                          newest max_delay words, q, the write position; the check that names the first refused index.

The a-priori bound of |y32 - y64| (reverb_bound), u = 2^-24, as the feature's issue states it: a line word takes
4 + log2 N roundings per sample (g s, q - v, the low-pass's fmaf, log2 N butterfly stages, the fmaf into the line), each
at most u times the largest line word of the float64 run, Lmax; a loop of gain 0.9 sums them as 1 / (1 - 0.9); an
output sees sum |c| of that, plus N + 1 roundings of its own sum (the product dry x and N fmafs), each at most u times
the largest partial sum, |dry| |x|max + sum |c| Lmax.  Derived, not measured; the figures of every case: pytest -s.

Without the feature every test here fails at the import of reverb_params / ReverbPlan or at the first gab_reverb_ call.
"""
import ctypes

import numpy as np
import pytest

from plan_helpers import bits
from test_mix_host import EPS, fma32, mix_ramp

f32 = np.float32
MIN_DELAY = 32
GMAX = {4: float.fromhex("0x1.ffffep-2"), 8: float.fromhex("0x1.6a09dp-2"), 16: float.fromhex("0x1.ffffep-3")}
DAMP_MAX = f32(1.0 - 2.0 ** -20)


def row_floats(N, O):
    return N * (3 + O) + 1


def identity(T, N, O):
    p = np.zeros((T, row_floats(N, O)), np.float32)
    p[:, -1] = 1.0
    return p


def make_row(N, O, g=0.0, damp=0.0, b=0.0, c=0.0, dry=1.0):
    """A row from scalars or per-line arrays; c: a scalar, [N] or [O][N]."""
    c = np.broadcast_to(np.asarray(c, np.float64), (O, N))
    parts = [np.broadcast_to(np.asarray(a, np.float64), (N,)) for a in (g, damp, b)] + [c.ravel(), [dry]]
    return np.concatenate(parts).astype(np.float32)


def hadamard_sign(r, k):
    return -1.0 if bin(r & k).count("1") & 1 else 1.0


def fma(a, b, c):
    """fma32, and where an operand is not finite what IEEE 754 says (fma32's error term means nothing there)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = fma32(a, b, c)
        plain = np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
    return np.where(np.isfinite(plain), r, plain.astype(np.float32)).astype(np.float32)


def sample_params(cur, tgt, ramp, B):
    """[P][T][B] float32: the target, or on a ramp buffer fmaf(target - current, r[s], current)."""
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    if ramp is None:
        return np.broadcast_to(tgt.T[:, :, None], (tgt.shape[1], tgt.shape[0], B))
    diff = (tgt - cur).T[:, :, None]                                  # float32: one rounding
    return fma(diff, np.asarray(ramp, np.float32)[None, None, :], cur.T[:, :, None])


def hadamard(u, N):
    """The butterflies of step 4 on u [T][N][...], in place, in the contract's stage order."""
    h = 1
    while h < N:
        for k in range(N):
            if not k & h:
                a, b = u[:, k].copy(), u[:, k + h].copy()
                u[:, k] = a + b
                u[:, k + h] = a - b
        h *= 2
    return u


def _run(x, delays, cur, tgt, ramp, hist, q, N, O, wide):
    x = np.asarray(x, np.float32)
    T, B = x.shape
    H = hist.shape[2]
    delays = np.asarray(delays, np.int64)
    assert delays.shape == (T, N) and delays.min() >= MIN_DELAY and delays.max() <= H
    ft = np.float64 if wide else np.float32
    p = sample_params(cur, tgt, ramp, B).astype(ft)
    g, damp, b = (np.swapaxes(p[k * N:(k + 1) * N], 0, 1) for k in range(3))      # [T][N][B]
    c = p[3 * N:(3 + O) * N].reshape(O, N, T, B)
    dry = p[-1]
    line = np.concatenate([np.asarray(hist, ft), np.zeros((T, N, B), ft)], axis=2)
    q = np.array(q, ft)
    xw = x.astype(ft)
    y = np.empty((T, O, B), ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for n0 in range(0, B, MIN_DELAY):
            n1 = min(B, n0 + MIN_DELAY)
            at = H + np.arange(n0, n1)[None, None, :] - delays[:, :, None]          # all < H + n0: before the block
            v = g[:, :, n0:n1] * np.take_along_axis(line, at, axis=2)
            Q = np.empty_like(v)
            for k in range(n1 - n0):
                d, vk = damp[:, :, n0 + k], v[:, :, k]
                q = d * (q - vk) + vk if wide else fma(d, q - vk, vk)
                Q[:, :, k] = q
            u = hadamard(Q.copy(), N)
            xb = xw[:, None, n0:n1]
            line[:, :, H + n0:H + n1] = b[:, :, n0:n1] * xb + u if wide else fma(b[:, :, n0:n1], xb, u)
            for o in range(O):
                acc = dry[:, n0:n1] * xw[:, n0:n1]
                for i in range(N):
                    ci = c[o, i][:, n0:n1]
                    acc = ci * Q[:, i] + acc if wide else fma(ci, Q[:, i], acc)
                y[:, o, n0:n1] = acc
    assert line.dtype == ft and q.dtype == ft and y.dtype == ft
    return y.reshape(T * O, B), line[:, :, B:], q, line[:, :, H:]


def reverb_reference_f32(x, delays, cur, tgt, ramp, hist, q, N, O):
    """x [T][B] float32, delays [T][N], cur / tgt [T][N (3 + O) + 1] float32; ramp: the table [B] on a buffer with a
    pending ramp, else None; hist [T][N][H]: the newest H >= max(delays) words of every line, the newest last; q [T][N].
    Returns (y [T O][B], hist afterwards, q afterwards), all float32."""
    y, hist, q, _ = _run(x, delays, cur, tgt, ramp, hist, q, N, O, False)
    return y, hist, q


def reverb_reference_f64(x, delays, cur, tgt, ramp, hist, q, N, O):
    y, hist, q, _ = _run(x, delays, cur, tgt, ramp, hist, q, N, O, True)
    return y, hist, q


def first_refused_param(table, N, O):
    """The flat index of the first value the contract refuses, or None."""
    t = np.asarray(table, np.float32).reshape(-1, row_floats(N, O))
    field = np.arange(t.shape[1])[None, :]
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(t)
        bad |= (field < N) & ~(np.abs(t) <= f32(GMAX[N]))
        bad |= (field >= N) & (field < 2 * N) & ~((t >= 0) & (t <= DAMP_MAX))
    hits = np.flatnonzero(bad.ravel())
    return int(hits[0]) if hits.size else None


def first_refused_delay(delays, max_delay):
    d = np.asarray(delays).ravel()
    hits = np.flatnonzero((d < MIN_DELAY) | (d > max_delay))
    return int(hits[0]) if hits.size else None


class Refused(ValueError):
    pass


class Twin:
    """The plan's state machine on the host; process() is reverb_reference_f32."""

    def __init__(self, T, B, N, O, max_delay):
        self.T, self.B, self.N, self.O, self.max_delay = T, B, N, O, max_delay
        self.cap = 1
        while self.cap < max_delay + 64:
            self.cap *= 2
        self.cur = identity(T, N, O)
        self.tgt = self.cur.copy()
        self.pending = False
        self.delays = np.full((T, N), max_delay, np.int32)
        self.reset()

    def set_params(self, p, ramp=True, first_track=0):
        p = np.asarray(p, np.float32).reshape(-1, row_floats(self.N, self.O))
        bad = first_refused_param(p, self.N, self.O)
        if bad is not None:
            raise Refused("track %d field %d" % (first_track + bad // p.shape[1], bad % p.shape[1]))
        self.tgt[first_track:first_track + p.shape[0]] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + p.shape[0]] = p

    def set_delays(self, d, first_track=0):
        d = np.asarray(d, np.int32).reshape(-1, self.N)
        bad = first_refused_delay(d, self.max_delay)
        if bad is not None:
            raise Refused("track %d line %d" % (first_track + bad // self.N, bad % self.N))
        self.delays[first_track:first_track + d.shape[0]] = d

    def reset(self):
        self.hist = np.zeros((self.T, self.N, self.max_delay), np.float32)
        self.q = np.zeros((self.T, self.N), np.float32)
        self.pos = 0
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x):
        y, self.hist, self.q = reverb_reference_f32(x, self.delays, self.cur, self.tgt,
                                                    mix_ramp(self.B) if self.pending else None, self.hist, self.q,
                                                    self.N, self.O)
        self.pos = (self.pos + self.B) % self.cap
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def reverb_mix(T, N, O, seed, loop=0.9):
    """Parameter rows that differ on neighbouring tracks and lines: loop gains up to `loop`, both signs, damping from
    none to heavy, input and output gains of both signs."""
    rng = np.random.RandomState(seed)
    p = np.zeros((T, row_floats(N, O)), np.float32)
    p[:, :N] = rng.uniform(0.3, loop, (T, N)) * GMAX[N] * rng.choice([-1.0, 1.0], (T, N))
    p[:, N:2 * N] = rng.uniform(0.0, 0.9, (T, N)) * (rng.uniform(0, 1, (T, N)) < 0.8)
    p[:, 2 * N:3 * N] = rng.uniform(-1.0, 1.0, (T, N))
    p[:, 3 * N:-1] = rng.uniform(-1.0, 1.0, (T, O * N)) / np.sqrt(N)
    p[:, -1] = rng.uniform(-1.0, 1.0, T)
    return p


def run_stream(x, delays, p, N, O, wide=False):
    """One long buffer x [T][n] at steady parameters from silence; returns (y [T O][n], the line words written)."""
    T = x.shape[0]
    H = int(np.max(delays))
    ft = np.float64 if wide else np.float32
    y, _, _, written = _run(x, delays, p, p, None, np.zeros((T, N, H), ft), np.zeros((T, N), ft), N, O, wide)
    return y, written


# ---- the Python surface, without a GPU ---------------------------------------------------------------------------
def test_reverb_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "ReverbPlan" in g.__all__ and callable(g.ReverbPlan) and "reverb_params" in g.__all__ and callable(g.reverb_params)
    for name in ("set_params", "set_delays", "reset", "process", "process_batch", "params", "state", "prepare", "launch",
                 "close"):
        assert hasattr(g.ReverbPlan, name), name


def test_row_floats_and_the_pinned_gain_limits():
    from gpuaudiobench_amd import _capi
    lib = _capi.lib
    for N in (4, 8, 16):
        for O in (1, 2):
            assert lib.gab_reverb_row_floats(N, O) == N * (3 + O) + 1
        want = np.float32((1.0 - 2.0 ** -20) / np.sqrt(np.float64(N)))    # float64 on the host, rounded once
        assert lib.gab_reverb_gmax(N) == float(want) == GMAX[N]
        assert float(want) * np.sqrt(np.float64(N)) < 1.0 - 2.0 ** -21
    for N, O in ((5, 1), (0, 1), (32, 2), (8, 0), (8, 3)):
        assert lib.gab_reverb_row_floats(N, O) == 0
    assert lib.gab_reverb_gmax(5) == 0.0


def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    # (tracks, bufsize, lines, outs, max_delay)
    for args in ((4, 512, 5, 2, 1000), (4, 512, 8, 3, 1000), (4, 512, 8, 2, 31), (0, 512, 8, 2, 1000), (-1, 512, 8, 2, 1000),
                 (4, 0, 8, 2, 1000), (4, 512, 0, 2, 1000), (4, 512, 32, 2, 1000), (4, 512, 8, 0, 1000),
                 (4, 512, 8, 2, (1 << 20) + 1)):
        assert lib.gab_reverb_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_reverb_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_reverb_create(None, 4, 512, 8, 2, 1000) == bad and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_reverb_process(None, None, None, None), b"gab_reverb_process"),
                       (lambda: lib.gab_reverb_process_batch(None, None, None, 1, None), b"gab_reverb_process_batch"),
                       (lambda: lib.gab_reverb_set_params(None, None, 1, None), b"gab_reverb_set_params"),
                       (lambda: lib.gab_reverb_set_params_tracks(None, None, 0, 1, 1, None), b"gab_reverb_set_params_tracks"),
                       (lambda: lib.gab_reverb_set_delays(None, None, None), b"gab_reverb_set_delays"),
                       (lambda: lib.gab_reverb_set_delays_tracks(None, None, 0, 1, None), b"gab_reverb_set_delays_tracks"),
                       (lambda: lib.gab_reverb_params(None, None, None, None), b"gab_reverb_params"),
                       (lambda: lib.gab_reverb_state(None, None, None, None, None, None), b"gab_reverb_state"),
                       (lambda: lib.gab_reverb_reset(None, None), b"gab_reverb_reset"),
                       (lambda: lib.gab_reverb_destroy(None), b"gab_reverb_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_reverb_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_reverb_create(C.byref(h), 4, 512, 8, 2, 1000)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_reverb_create" in text


# ---- exact known answers, independent of fma32 --------------------------------------------------------------------
def plain_network(x, m, g, c, n_out):
    """The contract at damp = 0, b = 1, dry = 1 with Python floats (float64) and a*b+c as two operations: one track,
    c [O][N].  For dyadic values that float32 holds every operation is exact, so no rounding rule enters."""
    N, O = len(m), len(c)
    H = max(m)
    line = [[0.0] * (H + len(x)) for _ in range(N)]
    y = [[0.0] * len(x) for _ in range(O)]
    for n in range(n_out):
        q = [g * line[i][H + n - m[i]] for i in range(N)]                 # damp = 0: q = 0 * (q - v) + v = v
        u = list(q)
        h = 1
        while h < N:
            for k in range(N):
                if not k & h:
                    u[k], u[k + h] = u[k] + u[k + h], u[k] - u[k + h]
            h *= 2
        for i in range(N):
            line[i][H + n] = 1.0 * x[n] + u[i]
        for o in range(O):
            acc = 1.0 * x[n]
            for i in range(N):
                acc = c[o][i] * q[i] + acc
            y[o][n] = acc
    return np.array(y, np.float64), np.array(line, np.float64)[:, H:]


@pytest.mark.parametrize("N,n", [(4, 600), (8, 400)])
def test_dyadic_impulses_are_exact(N, n):
    """g = 1 / N, c = +-0.5, impulses 3 and -2: every value is a dyadic rational that float32 holds over these samples,
    so float32, float64 and the restatement must agree on every bit."""
    m = (32, 34, 37, 41, 46, 52, 59, 67)[:N]
    c = [[0.5 * hadamard_sign(1 + o, i) for i in range(N)] for o in range(2)]
    x = np.zeros(600, np.float32)
    x[0], x[5] = 3.0, -2.0
    want, want_line = plain_network([float(v) for v in x], m, 1.0 / N, c, n)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)                 # float32 holds them: exact
    assert np.array_equal(want_line.astype(np.float32).astype(np.float64), want_line)
    p = make_row(N, 2, g=1.0 / N, b=1.0, c=c)[None, :]
    y, written = run_stream(x[None, :], np.array([m]), p, N, 2)
    assert np.array_equal(bits(y[:, :n]), bits(want[:, :n].astype(np.float32)))
    assert np.array_equal(bits(written[0][:, :n]), bits(want_line[:, :n].astype(np.float32)))
    y64, _ = run_stream(x[None, :], np.array([m]), p, N, 2, wide=True)
    assert np.array_equal(y64[:, :n], want[:, :n])
    nonzero = int(np.count_nonzero(want[:, :n]))
    print("N = %d: %d of %d outputs are not zero" % (N, nonzero, 2 * n))
    assert nonzero > n


# ---- first echoes ------------------------------------------------------------------------------------------------
def test_without_loop_gain_the_output_is_the_dry_path():
    N, O = 8, 2
    x = noise(3, 200, 1)
    p = np.tile(make_row(N, O, g=0.0, b=1.0, c=0.3, dry=0.75), (3, 1))
    y, _ = run_stream(x, np.full((3, N), 40), p, N, O)
    assert np.array_equal(bits(y.reshape(3, O, 200)), bits(np.repeat((f32(0.75) * x)[:, None, :], O, axis=1) + f32(0.0)))
    ident = identity(3, N, O)
    y, _ = run_stream(x, np.full((3, N), 40), ident, N, O)
    assert np.array_equal(bits(y.reshape(3, O, 200)), bits(np.repeat(x[:, None, :], O, axis=1)))


@pytest.mark.parametrize("N", [4, 8, 16])
def test_the_first_echo_of_one_line(N):
    """Only line i has b, g and c: a one-hot x comes back first at m[i] as c g b H[i][i]; a one-hot c on another line j
    picks out what H sends from i to j, one round trip later."""
    m = np.array([[33 + 3 * k for k in range(N)]])
    for i in (0, 1, N - 1):
        b, g, c = 0.5, 0.25, -0.75
        row = make_row(N, 1, g=np.eye(N)[i] * g, b=np.eye(N)[i] * b, c=np.eye(N)[i] * c, dry=0.0)[None, :]
        x = np.zeros((1, 200), np.float32)
        x[0, 7] = 1.0
        y, _ = run_stream(x, m, row, N, 1)
        first = np.flatnonzero(y[0])
        assert first[0] == 7 + m[0, i] and y[0, first[0]] == f32(c * g * b)                # q is tapped, H not yet seen
        assert first[1] == 7 + 2 * m[0, i] and y[0, first[1]] == f32(c * g * g * b * hadamard_sign(i, i))
        j = (i + 1) % N
        gj = np.eye(N)[i] * g + np.eye(N)[j] * g
        row = make_row(N, 1, g=gj, b=np.eye(N)[i] * b, c=np.eye(N)[j] * c, dry=0.0)[None, :]
        y, _ = run_stream(x, m, row, N, 1)
        first = np.flatnonzero(y[0])
        assert first[0] == 7 + m[0, i] + m[0, j] and y[0, first[0]] == f32(c * g * g * b * hadamard_sign(j, i))


# ---- decay time ----------------------------------------------------------------------------------------------------
def decay_time(y, fs, skip=0):
    """RT60 from the slope of the Schroeder integral between -5 and -35 dB."""
    e = np.cumsum((y[skip:].astype(np.float64) ** 2)[::-1])[::-1]
    db = 10.0 * np.log10(np.maximum(e / e[0], 1e-30))
    sel = np.flatnonzero((db <= -5.0) & (db >= -35.0))
    slope = np.polyfit(sel / fs, db[sel], 1)[0]
    return -60.0 / slope


@pytest.mark.parametrize("N", [4, 8, 16])
def test_decay_time(N):
    from gpuaudiobench_amd import reverb_params
    fs = 48000.0
    n = int(0.6 * fs)
    delays, table = reverb_params(rt60_s=0.5, lines=N, outs=1, fs=fs)
    assert delays[0, 0] in (1031, 1033) and 4700 <= delays[0, -1] <= 4900 and (np.diff(delays[0]) > 0).all()
    x = np.zeros((1, n), np.float32)
    x[0, 0] = 1.0
    y, _ = run_stream(x, delays, table, N, 1, wide=True)
    rt = decay_time(y[0, 1:], fs)
    print("N = %d: rt60 %.4f s for 0.5 s" % (N, rt))
    assert abs(rt / 0.5 - 1.0) <= 0.05
    # The Nyquist frequency decays as rt60_hf_s asks.  A burst of alternating signs under a 64-sample Hann window keeps
    # its energy within fs / 16 of the Nyquist frequency, where the one-pole is flat (a rectangular burst leaks into the
    # slower low band and reads 0.3 to 0.4 s).  A narrow band is a few modes beating, so the integral starts where every
    # line has come round twice and the network has mixed.
    delays, table = reverb_params(rt60_s=0.5, rt60_hf_s=0.25, lines=N, outs=1, fs=fs)
    burst = 64
    x = np.zeros((1, n), np.float32)
    x[0, :burst] = ((-1.0) ** np.arange(burst)) * np.hanning(burst)
    y, _ = run_stream(x, delays, table, N, 1, wide=True)
    rt = decay_time(y[0], fs, skip=burst + 2 * int(delays.max()))
    print("N = %d: rt60 %.4f s at the Nyquist frequency for 0.25 s" % (N, rt))
    assert abs(rt / 0.25 - 1.0) <= 0.05


# ---- float32 against float64 -----------------------------------------------------------------------------------
def reverb_bound(N, loop, sum_c, dry_x, Lmax):
    """The bound on |y32 - y64| of the module's docstring."""
    per_line = (4 + np.log2(N)) * EPS * Lmax / (1.0 - loop)
    return sum_c * per_line + (N + 1) * EPS * (dry_x + sum_c * Lmax)


@pytest.mark.parametrize("N", [4, 8, 16])
def test_float32_is_within_its_bound_of_float64(N):
    T, n, O, loop = 4, 4096, 2, 0.9
    rng = np.random.RandomState(40 + N)
    p = np.zeros((T, row_floats(N, O)), np.float32)
    p[:, :N] = loop * GMAX[N] * rng.choice([-1.0, 1.0], (T, N))
    p[:, N:2 * N] = rng.uniform(0.0, 0.9, (T, N))
    p[:, 2 * N:3 * N] = 1.0
    p[:, 3 * N:-1] = rng.uniform(-1.0, 1.0, (T, O * N)) / np.sqrt(N)
    p[:, -1] = 1.0
    delays = rng.randint(32, 400, (T, N))
    x = noise(T, n, 50 + N)
    y32, _ = run_stream(x, delays, p, N, O)
    y64, w64 = run_stream(x, delays, p, N, O, wide=True)
    Lmax = float(np.abs(w64).max())
    sum_c = float(np.abs(p[:, 3 * N:-1]).reshape(T, O, N).sum(axis=2).max())
    bound = reverb_bound(N, loop, sum_c, 1.0, Lmax)
    worst = float(np.abs(y32.astype(np.float64) - y64).max())
    print("N = %d: |y32 - y64| %.3g, bound %.3g (err / bound %.3g), largest line word %.3g, largest output %.3g"
          % (N, worst, bound, worst / bound, Lmax, float(np.abs(y64).max())))
    assert bound <= 1e-3 * float(np.abs(y64).max())                    # the bound itself means something
    assert worst <= bound


# ---- the check ---------------------------------------------------------------------------------------------------
def test_the_check_names_the_first_refused_index():
    N, O, T = 8, 2, 5
    P = row_floats(N, O)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))     # noqa: E731
    twin = Twin(T, 64, N, O, 1000)
    good = reverb_mix(T, N, O, 3)
    good[0, 0], good[1, 1], good[2, N] = GMAX[N], -GMAX[N], DAMP_MAX    # the edges themselves are admitted
    assert first_refused_param(good, N, O) is None
    for value, where in ((up(GMAX[N]), (1, 3)), (-up(GMAX[N]), (0, 0)), (1.0, (2, N + 1)), (f32(-1e-30), (3, 2 * N - 1)),
                         (up(DAMP_MAX), (0, N)), (np.nan, (4, 2 * N + 3)), (np.inf, (2, 3 * N)), (-np.inf, (3, P - 1)),
                         (np.nan, (1, N + 2)), (np.nan, (0, 5))):
        bad = good.copy()
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, P - 1] = np.nan                         # the FIRST offender is named
        assert first_refused_param(bad, N, O) == where[0] * P + where[1]
        with pytest.raises(Refused, match="track %d field %d$" % where):
            twin.set_params(bad)
        with pytest.raises(Refused, match="track %d field %d$" % where):
            twin.set_params(bad[where[0]:], first_track=where[0])
    assert np.array_equal(twin.tgt, identity(T, N, O)) and not twin.pending
    d = np.full((T, N), 500, np.int32)
    d[0, 0], d[4, 7] = 32, 1000
    assert first_refused_delay(d, 1000) is None
    for value, where in ((31, (2, 5)), (1001, (0, 1)), (0, (4, 0)), (-7, (3, 7))):
        bad = d.copy()
        bad[where] = value
        bad[4, 7] = 1001 if where != (4, 0) else 1000
        with pytest.raises(Refused, match="track %d line %d$" % where):
            twin.set_delays(bad)
    assert (twin.delays == 1000).all()


# ---- reverb_params -------------------------------------------------------------------------------------------------
PINNED_DELAYS = [487, 809, 1361, 2237]
PINNED_TABLE = [0x3ef17a0e, 0x3ee85461, 0x3ed97294, 0x3ec3c335, 0x3d6ef39d, 0x3dc6139e, 0x3e25ab1d, 0x3e86275f, 0x3f800000,
                0x3f800000, 0x3f800000, 0x3f800000, 0x3e009bcc, 0xbe009bcc, 0x3e009bcc, 0xbe009bcc, 0x3e009bcc, 0x3e009bcc,
                0xbe009bcc, 0xbe009bcc, 0x3f353bef]


def test_reverb_params():
    from gpuaudiobench_amd import reverb_params
    fs, N, O = 48000.0, 4, 2
    delays, table = reverb_params(rt60_s=1.2, rt60_hf_s=0.4, size_ms=10.0, lines=N, outs=O, wet_db=-12.0, dry_db=-3.0, fs=fs)
    assert delays.dtype == np.int32 and delays.shape == (1, N) and table.dtype == np.float32 and table.shape == (1, row_floats(N, O))
    m = delays[0].astype(np.float64)
    assert all(all(v % k for k in range(2, int(v ** 0.5) + 1)) for v in delays[0]) and (np.diff(delays[0]) > 0).all()
    assert delays[0, 0] >= 480 and delays[0, 0] < 500 and abs(delays[0, -1] / (480 * 4.65) - 1.0) < 0.02
    per_pass, per_pass_hf = 10.0 ** (-3.0 * m / (1.2 * fs)), 10.0 ** (-3.0 * m / (0.4 * fs))
    rho = per_pass_hf / per_pass
    wet = 10.0 ** (-12.0 / 20.0) / 2.0
    want = np.concatenate([per_pass / 2.0, (1.0 - rho) / (1.0 + rho), np.ones(N), wet * np.array([1, -1, 1, -1.0]),
                           wet * np.array([1, 1, -1, -1.0]), [10.0 ** (-3.0 / 20.0)]]).astype(np.float32)
    assert np.array_equal(bits(table[0]), bits(want))
    assert first_refused_param(table, N, O) is None
    # the pinned row
    assert delays[0].tolist() == PINNED_DELAYS and bits(table[0]).tolist() == PINNED_TABLE
    # per-track knobs, given delays, the plan's limits
    d, t = reverb_params([0.5, 1.0, 2.0], lines=8, outs=1, delays=[101, 211, 307, 401, 503, 601, 701, 809])
    assert d.shape == (3, 8) and t.shape == (3, row_floats(8, 1)) and (d == d[0]).all() and (t[0, :8] < t[1, :8]).all()
    assert (t[:, 8:16] == 0).all() and (t[:, -1] == 1).all()
    d, t = reverb_params(1e9, lines=16, outs=2)
    assert (t[0, :16] == f32(GMAX[16])).all()
    d, t = reverb_params(10.0, rt60_hf_s=1e-6, lines=4, outs=1)
    assert (t[0, 4:8] <= DAMP_MAX).all() and first_refused_param(t, 4, 1) is None
    for bad in (dict(rt60_s=0.0), dict(rt60_s=1.0, rt60_hf_s=2.0), dict(rt60_s=1.0, lines=5), dict(rt60_s=1.0, outs=3),
                dict(rt60_s=1.0, size_ms=0.0)):
        with pytest.raises(ValueError):
            reverb_params(**bad)
