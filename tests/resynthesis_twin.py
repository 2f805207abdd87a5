"""A numpy restatement of the resynthesis plan (include/gab_c_api.h, gab_resyn_*): which frames a call takes (the
spectrum plan's own counts, spectrum_twin), the dual window, and the overlap-add with its carried accumulator in float32
in the header's order.  The float32 transform is the packed-pair scipy.fft.ifft in complex64, as conv_pair_twin's are (a
yardstick for rounding, not a bit twin of the kernel's passes); the truth is np.fft.irfft in float64 of the same float32
rows.

So the overlap-add is an exact restatement (tests hold the kernel to it bit for bit, given the kernel's own u_j), and the
transform is held by a bound: per track and frame

    c = max_n |u - u64| / (peak_t + peak_p)

the peaks those of the float64 time-domain frames of the track and of its partner."""
import numpy as np

import conv_pair_twin as tw
import spectrum_twin as st

N, BINS = st.N, st.BINS
F32 = np.float32
LATENCY = N
MIN_HOP = st.MIN_HOP
C64_I = tw.C64(1j)

# which frames a call takes: the frames a spectrum plan of the same B, H and cut emits for it
count, counts, capacity, frame_ends = st.count, st.counts, st.capacity, st.frame_ends


# ---- the window ------------------------------------------------------------------------------------------------------
def dual_window64(w, H):
    """g[n] = w[n] / sum_m w[n + m H]^2, m over every index inside 0..1023 in ascending order; 0 where the sum is 0.
    float64 throughout, on w's values as they are."""
    w = np.asarray(w, np.float64)
    assert w.shape == (N,) and MIN_HOP <= H <= N
    g = np.zeros(N, np.float64)
    for r in range(H):
        s = 0.0
        for i in range(r, N, H):
            s += w[i] * w[i]
        if s != 0.0:
            g[r::H] = w[r::H] / s
    return g


def dual_window(w, H):
    """dual_window64, rounded once: what a new plan holds for w = spectrum_twin.window_hann()."""
    return dual_window64(w, H).astype(F32)


def bad_window(g):
    """The index of the first value that is not finite, else None.  (No rule on a sum.)"""
    bad = np.flatnonzero(~np.isfinite(np.asarray(g, F32)))
    return int(bad[0]) if bad.size else None


# ---- the overlap-add -------------------------------------------------------------------------------------------------
class Adder:
    """The plan's carried state, restated: the accumulator [T, 1024] and the position.  take(u [F, T, 1024], n) returns
    the call's output block [n, T, B] from the accumulator and the call's frames alone: v = g * u is one float32 product,
    and every slot adds its frames in ascending j, one float32 addition each."""

    def __init__(self, T, B, H, g):
        assert MIN_HOP <= H <= N
        self.T, self.B, self.H = T, B, H
        self.g = np.asarray(g, F32).copy()
        self.reset()

    def reset(self):
        self.acc = np.zeros((self.T, N), F32)
        self.p = 0

    def set_window(self, g):
        self.g = np.asarray(g, F32).copy()

    def count(self, n=1):
        return count(self.p, n * self.B, self.H)

    def take(self, u, n=1):
        L = n * self.B
        ends = frame_ends(self.p, L, self.H)
        u = np.asarray(u, F32).reshape(len(ends), self.T, N)
        y = np.concatenate([self.acc, np.zeros((self.T, L), F32)], axis=1)        # column i: y[p - N + i]
        with np.errstate(over="ignore", invalid="ignore"):
            for uj, e in zip(u, ends):
                s = e - self.p                                                    # the frame's first sample, jH - N
                v = self.g[None, :] * uj
                y[:, s:s + N] = y[:, s:s + N] + v
        assert y.dtype == F32
        self.acc = y[:, L:].copy()
        self.p += L
        return y[:, :L].reshape(self.T, n, self.B).transpose(1, 0, 2).copy()


def overlap_add(u, ends, g, total):
    """The whole stream at once, the frames u [F, T, 1024] that end at `ends` (ascending, the last <= total): (outputs
    [T, total], the accumulator [T, 1024] behind them)."""
    u = np.asarray(u, F32)
    T = u.shape[1]
    y = np.zeros((T, total + N), F32)                                             # column i: y[i - N]
    with np.errstate(over="ignore", invalid="ignore"):
        for uj, e in zip(u, ends):
            assert 0 < e <= total
            y[:, e:e + N] = y[:, e:e + N] + np.asarray(g, F32)[None, :] * uj
    return y[:, :total], y[:, total:]


# ---- the transform ---------------------------------------------------------------------------------------------------
def as_complex(rows):
    """[..., 513, 2] float32 -> complex64 [..., 513], bins 0 and 512 with their imaginary parts read as zero."""
    rows = np.asarray(rows, F32)
    X = np.empty(rows.shape[:-1], tw.C64)
    X.real, X.imag = rows[..., 0], rows[..., 1]
    X.imag[..., 0] = 0.0
    X.imag[..., BINS - 1] = 0.0
    return X


def as_rows(X):
    """complex [..., 513] -> float32 [..., 513, 2]."""
    X = np.asarray(X)
    return np.stack([X.real, X.imag], axis=-1).astype(F32)


def frames_f32(rows):
    """u [F, T, 1024] float32 of rows [F, T, 513, 2]: the packed-pair inverse in complex64.  Z[k] = Xa[k] + i Xb[k] for
    k <= 512, Z[N - k] = conj(Xa[k]) + i conj(Xb[k]) for 0 < k < 512; scipy's ifft carries the 2^-10."""
    from scipy import fft as sfft
    X = as_complex(rows)
    F, T, _ = X.shape
    pairs = (T + 1) // 2
    Xa = X[:, 0::2]
    Xb = np.zeros((F, pairs, BINS), tw.C64)
    Xb[:, :T // 2] = X[:, 1::2]
    Z = np.zeros((F, pairs, N), tw.C64)
    Z[..., :BINS] = Xa + C64_I * Xb
    Z[..., BINS:] = (np.conj(Xa) + C64_I * np.conj(Xb))[..., 1:BINS - 1][..., ::-1]
    z = sfft.ifft(Z, axis=-1)
    assert Z.dtype == z.dtype == tw.C64
    u = np.empty((F, 2 * pairs, N), F32)
    u[:, 0::2], u[:, 1::2] = z.real, z.imag
    return u[:, :T]


def truth(rows):
    """float64 frames of the float32 rows: [F, T, 1024]."""
    return np.fft.irfft(as_complex(rows).astype(np.complex128), n=N, axis=-1)


def figures(u, u64):
    """(c, level), each [F, T]: c = max_n |u - u64| / (peak_t + peak_p) on the time-domain peaks of the truth; nan
    where the level is zero."""
    u64 = np.asarray(u64, np.float64)
    peaks = np.abs(u64).max(axis=-1)
    level = np.stack([tw.pair_level(p) for p in peaks])
    err = np.abs(np.asarray(u, np.float64) - u64).max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(level > 0, err / level, np.nan)
    return c, level


# ---- the inputs the tests share --------------------------------------------------------------------------------------
def noise_rows(F, T, seed, lv=None):
    """[F, T, 513, 2] float32: seeded normal noise in every bin, track t at conv_pair_twin.levels(T)[t]."""
    lv = tw.levels(T) if lv is None else np.asarray(lv, np.float64)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, T, BINS, 2)) * lv[None, :, None, None]).astype(F32)


def analyse(x, H, w=None):
    """The analyser twin on the whole stream x [T, total]: rows [F, T, 513, 2] of the frames that end inside it."""
    frames = st.windowed(x, frame_ends(0, x.shape[1], H), st.window_hann() if w is None else w)
    return as_rows(st.spectra(frames))
