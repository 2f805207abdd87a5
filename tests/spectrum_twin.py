"""A numpy restatement of the spectrum plan (include/gab_c_api.h, gab_spec_*): the framing on a hop grid with carried
history, the window product in float32, and the power and band arithmetic in float32, exactly as the header writes
them.  The float32 transform is conv_pair_twin.fft_pair_twin (the packed-pair 1024-point r2c: a yardstick for rounding,
not a bit twin of the kernel's passes), the truth np.fft.rfft in float64 of the same float32 frames.

So the framing, the powers and the bands are exact restatements (tests hold the kernel to them bit for bit, given the
kernel's own complex bits), and the transform is held by a bound: per track and frame

    c = max_k |X - X64| / (peak_t + peak_p)

the peaks those of the float64 spectra of the track and of its partner in that frame."""
import math

import numpy as np

import conv_pair_twin as tw

N, BINS, HIST = 1024, 513, 1023
F32 = np.float32
MIN_HOP, MAX_BANDS = 32, 64


# ---- counts and framing ----------------------------------------------------------------------------------------------
def count(p, length, H):
    """Frames j with p < jH <= p + length."""
    return (p + length) // H - p // H


def counts(B, H, first_buffer, n):
    return [count(k * B, B, H) for k in range(first_buffer, first_buffer + n)]


def capacity(B, H, n):
    """The largest count a call of n buffers can return, at any position."""
    return -(-(n * B) // H)


def frame_ends(p, length, H):
    """The ends jH (one past the last sample) of the frames of a call that takes samples [p, p + length)."""
    return [j * H for j in range(p // H + 1, (p + length) // H + 1)]


def window_hann():
    """Periodic Hann, float64, rounded once."""
    n = np.arange(N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)).astype(F32)


def window_sum(w):
    """S: float64, added in ascending n."""
    S = 0.0
    for v in np.asarray(w, F32):
        S += float(v)
    return S


def inv_factors(S):
    """(inv for k = 0 and 512, inv for 0 < k < 512), each a float64 quotient rounded once."""
    with np.errstate(over="ignore"):
        return F32(1.0 / (S * S)), F32(4.0 / (S * S))


def inv_k(S):
    e, m = inv_factors(S)
    v = np.full(BINS, m, F32)
    v[0] = v[BINS - 1] = e
    return v


def windowed(x, ends, w):
    """x: [T, total] float32, the whole stream from sample 0.  Frames ending at `ends`: [F, T, 1024] float32, each
    value one float32 product; samples before 0 are zeros."""
    x = np.asarray(x, F32)
    T = x.shape[0]
    pad = np.concatenate([np.zeros((T, N), F32), x], axis=1)
    w = np.asarray(w, F32)
    out = np.empty((len(ends), T, N), F32)
    for i, e in enumerate(ends):
        assert 0 < e <= x.shape[1]
        out[i] = w[None, :] * pad[:, e:e + N]
    assert out.dtype == F32
    return out


class Framer:
    """The plan's carried state, restated: the last 1023 samples per track and the position.  take(block [n, T, B])
    returns the windowed frames [F, T, 1024] of the call from the history and the call alone."""

    def __init__(self, T, B, H, w=None):
        assert MIN_HOP <= H <= N
        self.T, self.B, self.H = T, B, H
        self.w = window_hann() if w is None else np.asarray(w, F32)
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.T, HIST), F32)
        self.p = 0

    def take(self, blocks):
        blocks = np.asarray(blocks, F32).reshape(-1, self.T, self.B)
        call = np.concatenate(list(blocks), axis=1)                       # [T, n B]
        length = call.shape[1]
        both = np.concatenate([self.hist, call], axis=1)                  # sample p - 1023 + i at column i
        ends = frame_ends(self.p, length, self.H)
        out = np.empty((len(ends), self.T, N), F32)
        for i, e in enumerate(ends):
            c = e - self.p + HIST                                         # column one past the frame's last
            assert c - N >= 0
            out[i] = self.w[None, :] * both[:, c - N:c]
        self.hist = both[:, -HIST:].copy()
        self.p += length
        return out


# ---- the transform, the powers, the bands ----------------------------------------------------------------------------
def spectra(frames):
    """[F, T, 1024] float32 -> complex64 [F, T, 513], the packed-pair float32 transform."""
    F, T, _ = frames.shape
    out = np.empty((F, T, BINS), tw.C64)
    for i in range(F):
        out[i] = tw.fft_pair_twin(frames[i].ravel(), T)
    return out


def truth(frames):
    """float64 spectra of the float32 frames: complex128 [F, T, 513]."""
    return np.fft.rfft(np.asarray(frames, np.float64), axis=-1)


def figures(X, X64):
    """(c, level), each [F, T]: per frame conv_pair_twin.fft_figures."""
    c, level = zip(*(tw.fft_figures(X[i], X64[i]) for i in range(len(X64))))
    return np.array(c).reshape(len(X64), -1), np.array(level).reshape(len(X64), -1)


def powers(X, S):
    """P[k] = (re re + im im) inv_k in float32, every operation rounded once.  X: complex64 [..., 513] or float32
    [..., 513, 2]."""
    if np.iscomplexobj(X):
        re, im = np.asarray(X.real, F32), np.asarray(X.imag, F32)
    else:
        X = np.asarray(X, F32)
        re, im = X[..., 0], X[..., 1]
    with np.errstate(over="ignore", invalid="ignore"):
        P = (re * re + im * im) * inv_k(S)
    assert P.dtype == F32
    return P


def band_sums(P, edges):
    """Band b = the float32 sum of P[..., k], e_b <= k < e_(b+1), in ascending k from 0.0f."""
    P = np.asarray(P, F32)
    out = np.zeros(P.shape[:-1] + (len(edges) - 1,), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(len(edges) - 1):
            acc = np.zeros(P.shape[:-1], F32)
            for k in range(edges[b], edges[b + 1]):
                acc = acc + P[..., k]
            out[..., b] = acc
    assert out.dtype == F32
    return out


# ---- the rules -------------------------------------------------------------------------------------------------------
def default_edges(bands):
    return [BINS * b // bands for b in range(bands + 1)]


def bad_edge(edges, bands):
    """The index of the first edge that breaks 0 <= e_0 < e_1 < ... < e_bands <= 513, or -1."""
    assert len(edges) == bands + 1
    for b, e in enumerate(edges):
        if e < 0 or e > BINS or (b > 0 and e <= edges[b - 1]):
            return b
    return -1


def bad_window(w):
    """The index of the first value that is not finite; "sum" for a table of finite values whose S is zero; else
    None."""
    w = np.asarray(w, F32)
    bad = np.flatnonzero(~np.isfinite(w))
    if bad.size:
        return int(bad[0])
    return "sum" if window_sum(w) == 0.0 else None


# ---- the inputs the tests share --------------------------------------------------------------------------------------
def noise(T, total, seed, lv=None):
    """[T, total] float32: seeded normal noise, track t at conv_pair_twin.levels(T)[t] (powers of two: exact)."""
    lv = tw.levels(T) if lv is None else np.asarray(lv, np.float64)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, total)) * lv[:, None]).astype(F32)


def blocks(x, B):
    """[T, n B] -> [n, T, B]: the stream cut into buffers, track-major per buffer."""
    T, total = x.shape
    assert total % B == 0
    return x.reshape(T, total // B, B).transpose(1, 0, 2).copy()          # (a copy: x may be read-only)


def one_hot(n0):
    w = np.zeros(N, F32)
    w[n0] = 1.0
    return w


def one_hot_answer(x, ends, n0):
    """The closed form under a one-hot window at n0: X[k] = x[e - N + n0] exp(-2 pi i k n0 / N), [F, T, 513]."""
    x = np.asarray(x, np.float64)
    k = np.arange(BINS)
    ph = np.exp(-2j * np.pi * ((k * n0) % N) / N)
    out = np.zeros((len(ends), x.shape[0], BINS), np.complex128)
    for i, e in enumerate(ends):
        a = e - N + n0
        if a >= 0:
            out[i] = x[:, a][:, None] * ph[None, :]
    return out


def ordered_sum_bound(values):
    """The a-priori bound of an ordered float32 sum of n non-negative terms against the exact sum: (n - 1) u sum,
    u = 2^-24 (each of the n - 1 additions rounds a partial sum that is at most the whole), first order."""
    n = len(values)
    return (n - 1) * 2.0 ** -24 * math.fsum(values) * (1.0 + n * 2.0 ** -24)
