"""A plain float32 restatement of the packed-pair arithmetic of the FFT convolution routes and of gab_fft_r2c_1024:
the yardstick the per-channel gates (test_conv_levels_gpu.py, test_fft_levels_gpu.py, tools/conv_levels.py) measure
the kernels against.  numpy / scipy.fft only, complex64 throughout (asserted at every step).

The kernels pack channels 2q and 2q + 1 into one complex transform, z = x_a + i x_b.  With Z'[k] = conj(Z[N - k]) the
packed output's spectrum is W = Z P + Z' M, P = (Ha + Hb) / 2, M = (Ha - Hb) / 2; real(ifft W) = y_a, imag = y_b.
Every rounding error of that chain is relative to |Z| |P| + |Z'| |M|, the PAIR's level, and lands on both channels:
a channel's absolute error follows its pair, not itself.  The figure per channel is therefore

    c_t = max |y_t - truth_t| / (peak_t + peak_p)        p the partner (a zero partner for an odd last channel)

with the peaks those of the float64 truth over the whole stream.  c_twin is the largest c_t of this yardstick.

A route is described by its cut: a list of (first tap, end tap, transform size).  Partitions of equal transform size
are summed in the spectrum before one inverse, as the kernels do (classic: two sizes, two inverses; split: A and A2
share one; uniform and fdl: one inverse per buffer).  This is a yardstick for rounding, not a bit twin: scipy's
transform is not the kernels' radix-16 / radix-4 passes, and the split cut's far share is computed in place here,
not one buffer ahead."""
import math

import numpy as np

C64 = np.complex64
LEVELS = (1.0, 2.0 ** -10, 1.0, 0.0, 2.0 ** -20, 2.0 ** -20, 1.0, 1.0)     # loud/quiet, loud/silent, quiet/quiet, loud/loud
PAIRED = ("classic", "bank", "split", "fused", "uniform", "fdl")
EDGES_512 = (0, 511, 512, 1023, 1024, 2047, 2048, 4095)


def levels(T):
    return np.array([LEVELS[t % len(LEVELS)] for t in range(T)])


def route_cut(kind, B, L):
    """The (first tap, end tap, transform size) list of a route (k_conv_accel.hip, k_conv_fdl.hip); None: direct."""
    if kind == "direct":
        return None
    if kind == "fused" or (kind in ("classic", "bank") and L <= 512):
        return [(0, min(L, 512), 1024)]
    if kind in ("classic", "bank"):                       # partition A on 1024 points, partition B on 4096
        return [(0, 512, 1024), (512, min(L, 4096), 4096)]
    if kind == "split":                                   # A, A2 (one inverse), F
        return [(0, 512, 1024), (512, 1024, 1024), (1024, 4096, 4096)]
    if kind == "uniform":                                 # partition 0 of B taps, then S = 4096 - B each, all on 4096
        S = 4096 - B
        J = 1 + (-(-(L - B) // S) if L > B else 0)
        return [(0, min(L, B), 4096)] + [(B + (p - 1) * S, min(L, B + p * S), 4096) for p in range(1, J)]
    assert kind == "fdl"
    return [(p * B, min(L, (p + 1) * B), 2 * B) for p in range(math.ceil(L / B))]


def edge_taps(kind, B, L):
    """The one-hot taps of the known-answer case: the route's partition edges."""
    if kind in ("classic", "bank", "split"):
        return [k for k in EDGES_512 if k < L]
    cut = route_cut(kind, B, L)
    taps = {0, B - 1, B, L - 1}
    for f, e, _ in cut or []:
        taps |= {f, e - 1}
    return sorted(k for k in taps if 0 <= k < L)


def nan_stay(kind, B, L):
    """Buffers (the struck one included) whose transforms hold a sample: a NaN stays in its pair that long, derived
    from the route's history as test_conv_plan_state_gpu.wrap_len is.
    fused: the window [k-1 | k].  classic: partition B's window is the whole ring, the eight previous blocks, so the
    struck buffer and wrap_len more.  split: F of block k holds the ring's seven newest blocks and block k and makes
    the far share of blocks k+1 and k+2, for a pair every other buffer: one buffer more.  uniform: the last
    partition's 4096-sample window ends B + (J-2) S samples before the newest.  fdl: the spectra of the windows
    [i-1 | i] and [i | i+1] leave the K partitions after buffer i + K.  direct: the L - 1 samples of history."""
    from test_conv_plan_state_gpu import wrap_len
    if kind == "fused" or (kind in ("classic", "bank") and L <= 512):
        return 2
    if kind in ("classic", "bank"):
        return 1 + wrap_len(2, B, L, kind)
    if kind == "split":
        return 2 + wrap_len(2, B, L, kind)
    if kind == "uniform":
        return (4096 + route_cut(kind, B, L)[-1][0]) // B
    if kind == "fdl":
        return math.ceil(L / B) + 1
    return -(-(L - 1) // B) + 1


def decaying_ir(T, L, B, seed, level=1.0):
    """Independent noise per channel under exp(-n / B): partition 0 carries 86 % of the energy, and neighbouring
    channels share nothing, so M = (Ha - Hb) / 2 is as large as P."""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((T, L)) * np.exp(-np.arange(L) / float(B)) * level
    return h.astype(np.float32).ravel()


def noise(T, B, n, seed, lv=None):
    """n buffers [T*B] of seeded normal noise, channel t scaled by lv[t] (powers of two: exact)."""
    rng = np.random.default_rng(seed)
    lv = np.ones(T) if lv is None else np.asarray(lv, np.float64)
    return [(rng.standard_normal((T, B)) * lv[:, None]).astype(np.float32).ravel() for _ in range(n)]


def _pack(a, T, width):
    """[T*width] channel-major -> complex64 [pairs, width], an odd last channel beside zeros."""
    a = np.asarray(a, np.float32).reshape(T, width)
    pairs = (T + 1) // 2
    z = np.zeros((pairs, width), C64)
    z.real = a[0::2]
    z.imag[:T // 2] = a[1::2]
    return z


def _mirror(Z):
    """Z'[k] = conj(Z[(N - k) mod N]) along the last axis."""
    return np.conj(np.roll(Z[..., ::-1], 1, axis=-1))


def pair_spectra(ir, T, L, cut):
    """[(P, M)] per partition, complex64 [pairs, N] each (None for a partition whose taps are all zero)."""
    from scipy import fft as sfft
    h = _pack(ir, T, L)
    out = []
    for f, e, N in cut:
        g = np.zeros((h.shape[0], N), C64)
        g[:, :e - f] = h[:, f:e]
        if not g.any():
            out.append(None)
            continue
        Z = sfft.fft(g, axis=-1)
        Zm = _mirror(Z)
        Ha, Hb = (Z + Zm) * np.float32(0.5), (Z - Zm) * C64(-0.5j)
        P, M = (Ha + Hb) * np.float32(0.5), (Ha - Hb) * np.float32(0.5)
        assert Z.dtype == P.dtype == M.dtype == C64
        out.append((P, M))
    return out


def pair_stream(xs, ir, T, B, L, cut):
    """The packed-pair overlap-save of `cut` over the stream xs (n buffers [T*B], channel-major) in float32:
    n outputs [B*T], sample-major (out[s*T + t]) like the plan's."""
    from scipy import fft as sfft
    for f, e, N in cut:
        assert 0 < e - f <= N - B + 1, (f, e, N)          # the last B outputs of the circular product are linear
    n, pairs = len(xs), (T + 1) // 2
    pad = max(N + f for f, _, N in cut)
    X = np.zeros((pairs, pad + n * B), C64)
    for k, x in enumerate(xs):
        X[:, pad + k * B: pad + (k + 1) * B] = _pack(x, T, B)
    pm = pair_spectra(ir, T, L, cut)
    sizes = sorted({N for _, _, N in cut})
    out = []
    for k in range(n):
        y = np.zeros((pairs, B), C64)
        for N in sizes:
            W = None
            for (f, e, Np), s in zip(cut, pm):
                if Np != N or s is None:
                    continue
                end = pad + (k + 1) * B - f               # the window ends f samples before the newest
                Z = sfft.fft(X[:, end - N:end], axis=-1)
                w = Z * s[0] + _mirror(Z) * s[1]
                assert Z.dtype == w.dtype == C64
                W = w if W is None else W + w
            if W is not None:
                t = sfft.ifft(W, axis=-1)
                assert t.dtype == C64
                y = y + t[:, N - B:]
        assert y.dtype == C64
        o = np.empty((B, 2 * pairs), np.float32)
        o[:, 0::2], o[:, 1::2] = y.real.T, y.imag.T
        out.append(np.ascontiguousarray(o[:, :T]).ravel())
    return out


def direct_stream(xs, ir, T, B, L):
    """The direct route's float32 restatement: one accumulator per output, taps ascending, one rounding per tap
    (the kernel's fused multiply-add: a float32 product is exact in float64, the sum is rounded to float32 once)."""
    n = len(xs)
    X = np.zeros((T, L + n * B), np.float64)
    for k, x in enumerate(xs):
        X[:, L + k * B: L + (k + 1) * B] = np.asarray(x, np.float32).reshape(T, B)
    h = np.asarray(ir, np.float32).reshape(T, L).astype(np.float64)
    acc = np.zeros((T, n * B), np.float32)
    for k in range(L):
        acc = (acc + X[:, L - k: L - k + n * B] * h[:, k:k + 1]).astype(np.float32)
    assert acc.dtype == np.float32
    return [np.ascontiguousarray(acc[:, i * B:(i + 1) * B].T).ravel() for i in range(n)]


def twin_stream(kind, xs, ir, T, B, L):
    cut = route_cut(kind, B, L)
    return direct_stream(xs, ir, T, B, L) if cut is None else pair_stream(xs, ir, T, B, L, cut)


def per_channel(ys, T, B):
    """n outputs [B*T] sample-major -> [T, n, B]."""
    return np.stack([np.asarray(y).reshape(B, T).T for y in ys], axis=1)


def pair_level(peaks, paired=True):
    """peak_t + peak_p per channel (peak_t alone where nothing is packed)."""
    peaks = np.asarray(peaks, np.float64)
    if not paired:
        return peaks.copy()
    T = peaks.size
    partner = np.array([peaks[t ^ 1] if (t ^ 1) < T else 0.0 for t in range(T)])
    return peaks + partner


def channel_figures(ys, truths, T, B, first=0, paired=True):
    """(c, level): c_t = max |y_t - truth_t| over buffers >= first, over level_t = peak_t + peak_p, the peaks those
    of the truth over the whole stream.  c_t is nan where the level is zero (a silent pair: nothing to divide by)."""
    y, r = per_channel(ys, T, B).astype(np.float64), per_channel(truths, T, B)
    level = pair_level(np.abs(r).max(axis=(1, 2)), paired)
    err = np.abs(y - r)[:, first:].max(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(level > 0, err / level, np.nan)
    return c, level


def c_max(c):
    return float(np.nanmax(c))


# ---- the inputs the gates share -----------------------------------------------------------------------------------
# The ten shapes of the gates: route ids of test_conv_plan_state_gpu.ROUTES, the smallest that reach each kernel.
LEVEL_ROUTES = ("split", "classic-T6", "classic-T8", "fused-notail", "uniform-256", "uniform-1024", "uniform-32",
                "direct", "fdl", "fdl-groups")


def stream_len(T, B, L, kind):
    from test_conv_plan_state_gpu import fill_len, wrap_len
    return fill_len(B, L) + wrap_len(T, B, L, kind) + 4


def levels_case(T, B, L, kind, lv=None, seed=1):
    """(ir, xs): the unequal-levels stream of a route, channel t's input at lv[t] (default: levels(T))."""
    lv = levels(T) if lv is None else lv
    return decaying_ir(T, L, B, seed), noise(T, B, stream_len(T, B, L, kind), seed + 100, lv)


def one_hot_cases(T, B, L, kind):
    """[(taps, ir)]: one-hot responses, channel t's only tap at taps[t]; every edge tap of the route in turn."""
    edges = edge_taps(kind, B, L)
    cases = []
    for i in range(0, len(edges), T):
        taps = [edges[(i + t) % len(edges)] for t in range(T)]
        ir = np.zeros((T, L), np.float32)
        ir[np.arange(T), taps] = 1.0
        cases.append((taps, ir.ravel()))
    return cases


def delayed(xs, taps, T, B):
    """The stream delayed by taps[t] samples on channel t: n outputs [B*T], sample-major (exact)."""
    n = len(xs)
    X = np.stack([np.asarray(x, np.float32).reshape(T, B) for x in xs], axis=1).reshape(T, n * B)
    Y = np.zeros_like(X)
    for t, d in enumerate(taps):
        Y[t, d:] = X[t, :n * B - d]
    return [np.ascontiguousarray(Y[:, i * B:(i + 1) * B].T).ravel() for i in range(n)]


# ---- the 1024-point r2c ---------------------------------------------------------------------------------------------
def fft_pair_twin(x, T):
    """Packed-pair float32 1024-point r2c: [T*1024] -> complex64 [T, 513]."""
    from scipy import fft as sfft
    Z = sfft.fft(_pack(x, T, 1024), axis=-1)
    Zm = _mirror(Z)
    Xa, Xb = (Z + Zm) * np.float32(0.5), (Z - Zm) * C64(-0.5j)
    assert Z.dtype == Xa.dtype == Xb.dtype == C64
    out = np.empty((2 * Z.shape[0], 513), C64)
    out[0::2], out[1::2] = Xa[:, :513], Xb[:, :513]
    return out[:T]


def fft_truth(x, T):
    return np.fft.rfft(np.asarray(x, np.float64).reshape(T, 1024), axis=-1)


def fft_figures(X, truth, paired=True):
    """(c, level) per track of a [T, 513] spectrum: the largest bin error over the pair's spectral peaks."""
    truth = np.asarray(truth)
    level = pair_level(np.abs(truth).max(axis=1), paired)
    err = np.abs(np.asarray(X, np.complex128) - truth).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(level > 0, err / level, np.nan)
    return c, level


FFT_IMPULSES, FFT_COSINES = (0, 1, 511, 512, 1023), (1, 255, 256, 511)


def fft_known_answers(T):
    """(x [T, 1024], want [T, 513]): track t takes signal (t + T) mod 11 of: unit impulses at FFT_IMPULSES (modulus 1
    in every bin, phase -2 pi k n / N), DC, the alternating +-1 sequence (bin 512 only), cosines on FFT_COSINES (that
    bin only); scaled so that every spectral peak is 1 (an impulse's bins beside an unscaled cosine's 512 would be
    2e-3 of the pair's peak).  Neighbours in a pair are different signals: each one's leakage into its partner shows."""
    n, k = np.arange(1024), np.arange(513)
    signals = [((n == m).astype(np.float64), np.exp(-2j * np.pi * ((k * m) % 1024) / 1024)) for m in FFT_IMPULSES]
    signals.append((np.ones(1024) / 1024, (k == 0).astype(complex)))
    signals.append((np.where(n % 2 == 0, 1.0, -1.0) / 1024, (k == 512).astype(complex)))
    signals += [(np.cos(2 * np.pi * b * n / 1024) / 512, (k == b).astype(complex)) for b in FFT_COSINES]
    pick = [signals[(t + T) % len(signals)] for t in range(T)]
    return np.stack([p[0] for p in pick]), np.stack([p[1] for p in pick])
