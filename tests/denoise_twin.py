"""A numpy restatement of the denoise plan (include/gab_c_api.h, gab_dn_*): the spectrum plan's framing and powers
(spectrum_twin), the gate per (track, bin) in float32 with a one-rounding fma32 (test_mix_host's, checked there against
exact rational arithmetic), and the resynthesis plan's packing and overlap-add (resynthesis_twin).

The gate is an exact restatement: given the device's own complex bins, tests hold the rows form to it bit for bit.  The
two transforms are the twins' (yardsticks for rounding, not bit twins of the kernel's passes), so the fused form is held
to the composition of the three plans on the device bit for bit, and to the float64 truth below by a bound."""
import numpy as np

import resynthesis_twin as rt
import spectrum_twin as st
from test_mix_host import fma32

N, BINS, HIST = st.N, st.BINS, st.HIST
F32 = np.float32
FIELDS = ("floor", "att", "rel")
LATENCY = N
ONE = F32(1.0)


# ---- the gate --------------------------------------------------------------------------------------------------------
def gate_step(re, im, m, thr, inv, floor, att, rel):
    """One frame of the header's five lines on arrays of bins: (re', im', m', P, tg).  float32, every operation rounded
    once, one fma."""
    re, im, m = np.asarray(re, F32), np.asarray(im, F32), np.asarray(m, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        P = ((re * re) + (im * im)) * np.asarray(inv, F32)
        assert P.dtype == F32
        tg = np.where(P > np.asarray(thr, F32), ONE, np.asarray(floor, F32)).astype(F32)     # strict; NaN compares false
        c = np.where(tg > m, np.asarray(att, F32), np.asarray(rel, F32)).astype(F32)
        m2 = fma32(c, (m - tg).astype(F32), tg)
        return (m2 * re).astype(F32), (m2 * im).astype(F32), m2, P, tg


def default_params(T):
    p = np.zeros((T, 3), F32)
    p[:, 0] = 1.0
    return p


class Gate:
    """The rows form: the carried mask [T, 513] and the two tables.  take(rows [F, T, 513, 2]) returns the gated rows
    and advances the mask, frame by frame in ascending order."""

    def __init__(self, T, w=None):
        self.T = T
        self.inv = st.inv_k(st.window_sum(st.window_hann() if w is None else w))
        self.thr = np.zeros((T, BINS), F32)
        self.params = default_params(T)
        self.reset()

    def reset(self):
        self.mask = np.ones((self.T, BINS), F32)

    def set_window(self, w):
        self.inv = st.inv_k(st.window_sum(w))

    def set_thresholds(self, thr, first_track=0):
        thr = np.asarray(thr, F32).reshape(-1, BINS)
        assert bad_threshold(thr) is None
        self.thr[first_track:first_track + len(thr)] = thr

    def set_params(self, rows, first_track=0):
        rows = np.asarray(rows, F32).reshape(-1, 3)
        assert bad_param(rows) is None
        self.params[first_track:first_track + len(rows)] = rows

    def take(self, rows):
        rows = np.asarray(rows, F32).reshape(-1, self.T, BINS, 2)
        out = np.empty_like(rows)
        fl, at, rl = (self.params[:, i][:, None] for i in range(3))
        for f in range(len(rows)):
            out[f, ..., 0], out[f, ..., 1], self.mask, _, _ = gate_step(rows[f, ..., 0], rows[f, ..., 1], self.mask,
                                                                        self.thr, self.inv[None, :], fl, at, rl)
        return out


class Denoiser:
    """The fused form, restated as the header's composition: spectrum_twin's Framer and transform, Gate,
    resynthesis_twin's transform and Adder.  process(blocks [n, T, B]) returns [n, T, B]; the four carried states are
    hist, acc, mask and the position."""

    def __init__(self, T, B, H, w=None, g=None):
        w = st.window_hann() if w is None else np.asarray(w, F32)
        g = rt.dual_window(st.window_hann(), H) if g is None else np.asarray(g, F32)
        self.T, self.B, self.H = T, B, H
        self.framer, self.gate, self.adder = st.Framer(T, B, H, w), Gate(T, w), rt.Adder(T, B, H, g)

    def reset(self):
        self.framer.reset()
        self.gate.reset()
        self.adder.reset()

    hist = property(lambda self: self.framer.hist)
    acc = property(lambda self: self.adder.acc)
    mask = property(lambda self: self.gate.mask)
    p = property(lambda self: self.adder.p)

    def process(self, blocks):
        blocks = np.asarray(blocks, F32).reshape(-1, self.T, self.B)
        rows = rt.as_rows(st.spectra(self.framer.take(blocks)))
        gated = self.gate.take(rows)
        u = rt.frames_f32(gated) if len(gated) else np.zeros((0, self.T, N), F32)
        assert self.framer.p == self.adder.p + len(blocks) * self.B
        return self.adder.take(u, len(blocks))


# ---- the float64 truth -----------------------------------------------------------------------------------------------
def truth64(x, H, thr, params, w=None, g=None):
    """The whole stream x [T, total] through the chain in float64 on the float32 tables' values: windowed float32 frames,
    rfft, the gate with P, tg, c and m in float64, irfft, the synthesis window, overlap-add.  Returns (y [T, total] with
    the 1024 samples of latency, P64 [F, T, 513])."""
    w = st.window_hann() if w is None else w
    g = rt.dual_window(st.window_hann(), H) if g is None else g
    T, total = x.shape
    ends = rt.frame_ends(0, total, H)
    X = st.truth(st.windowed(x, ends, w))
    inv = st.inv_k(st.window_sum(w)).astype(np.float64)
    thr, params = np.asarray(thr, np.float64), np.asarray(params, np.float64)
    fl, at, rl = (params[:, i][:, None] for i in range(3))
    m = np.ones((T, BINS))
    P64 = np.empty(X.shape)
    for f in range(len(X)):
        P64[f] = (X[f].real ** 2 + X[f].imag ** 2) * inv[None, :]
        tg = np.where(P64[f] > thr, 1.0, fl)
        c = np.where(tg > m, at, rl)
        m = c * (m - tg) + tg
        X[f] = X[f] * m
    X[..., 0] = X[..., 0].real
    X[..., BINS - 1] = X[..., BINS - 1].real
    v = np.fft.irfft(X, n=N, axis=-1) * np.asarray(g, np.float64)[None, None, :]
    y = np.zeros((T, total + N))
    for vj, e in zip(v, ends):
        y[:, e:e + N] += vj
    return y[:, :total], P64


def powers64(x, H, w=None):
    """P64 [F, T, 513] of the whole stream x: the float64 powers that truth64 compares with the thresholds."""
    w = st.window_hann() if w is None else w
    X = st.truth(st.windowed(x, rt.frame_ends(0, x.shape[1], H), w))
    return (X.real ** 2 + X.imag ** 2) * st.inv_k(st.window_sum(w)).astype(np.float64)[None, None, :]


def thresholds_clear_of(P64):
    """thr [T, 513] float32 that no decision can flip on: per (track, bin), the geometric mean of the two powers, adjacent
    in sorted order over the frames and inside its middle half, that lie furthest apart in ratio.  So every bin opens in
    a quarter of the frames at least and shuts in a quarter at least, and no power lies near its threshold (the callers
    assert the margin)."""
    logs = np.sort(np.log(np.maximum(P64, 1e-300)), axis=0)
    F = len(logs)
    gap = np.diff(logs, axis=0)[F // 4:3 * F // 4]
    i = gap.argmax(axis=0)[None] + F // 4
    mid = 0.5 * (np.take_along_axis(logs, i, axis=0) + np.take_along_axis(logs, i + 1, axis=0))[0]
    return np.exp(mid).astype(F32)


def clear_of_thresholds(P64, thr, margin=1e-3):
    """Does no power lie within a factor 1 +- margin of its threshold?"""
    thr = np.asarray(thr, np.float64)[None]
    return not ((P64 > thr * (1 - margin)) & (P64 < thr * (1 + margin))).any()


def accuracy_case(T, total, H, seed):
    """(x, thr, params) for the accuracy rule: unit noise under a few tones a track, thresholds_clear_of its own float64
    powers, and a glide with a floor."""
    rng = np.random.default_rng(seed)
    n = np.arange(total)
    x = rng.uniform(-1.0, 1.0, (T, total))
    for t in range(T):
        for k in rng.choice(np.arange(8, 500), 3, replace=False):
            x[t] += 0.5 * np.sin(2.0 * np.pi * k * n / N + rng.uniform(0, 6.28))
    x = x.astype(F32)
    params = np.tile(np.array([0.1, 0.3, 0.7], F32), (T, 1))
    return x, thresholds_clear_of(powers64(x, H)), params


def pair_err(y, ref):
    """max |y - ref| per pair of tracks: a track's absolute error follows its pair's."""
    e = np.abs(np.asarray(y, np.float64) - ref).max(axis=1)
    e = np.concatenate([e, np.zeros(len(e) % 2)])
    return e.reshape(-1, 2).max(axis=1)


def stream_of(blocks_out):
    """[n, T, B] -> [T, n B]."""
    n, T, B = blocks_out.shape
    return blocks_out.transpose(1, 0, 2).reshape(T, n * B)


# ---- the rules -------------------------------------------------------------------------------------------------------
def bad_threshold(thr):
    """The flat index of the first value that is a NaN or negative (+inf is allowed), else None."""
    t = np.asarray(thr, F32).ravel()
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(~(t >= 0))
    return int(bad[0]) if bad.size else None


def bad_param(rows):
    """The flat index of the first value outside 0 <= floor <= 1, 0 <= att < 1, 0 <= rel < 1 (a NaN is), else None."""
    r = np.asarray(rows, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = (r >= 0) & np.stack([r[:, 0] <= 1, r[:, 1] < 1, r[:, 2] < 1], axis=1)
    bad = np.flatnonzero(~ok.ravel())
    return int(bad[0]) if bad.size else None


def threshold_refusal(i, first_track=0):
    return "track %d bin %d (threshold) must be >= 0 or +inf, not a NaN; the plan keeps its thresholds" % (
        first_track + i // BINS, i % BINS)


def param_refusal(i, first_track=0):
    rule = "must be within [0, 1]" if i % 3 == 0 else "must be within [0, 1)"
    return "track %d field %d (%s) %s; the plan keeps its parameters" % (first_track + i // 3, i % 3, FIELDS[i % 3], rule)


# ---- the tables the tests share --------------------------------------------------------------------------------------
def seeded_tables(T, seed, level=1.0):
    """(thr [T, 513] around the power `level` of a bin, two decades wide, with a few zeros and +inf; params [T, 3])."""
    rng = np.random.default_rng(seed)
    thr = (level * 10.0 ** rng.uniform(-1.0, 1.0, (T, BINS))).astype(F32)
    thr[rng.random((T, BINS)) < 0.03] = 0.0
    thr[rng.random((T, BINS)) < 0.03] = np.inf
    params = np.stack([rng.uniform(0.0, 1.0, T), rng.uniform(0.0, 0.95, T), rng.uniform(0.0, 0.95, T)], axis=1).astype(F32)
    if T > 1:
        params[rng.integers(T)] = 0.0, 0.0, 0.0                          # a hard gate on one track
    return thr, params
