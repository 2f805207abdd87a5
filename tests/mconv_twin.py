"""The matrix-convolution plan's contract restated in numpy (include/gab_c_api.h, gab_mconv_*), without a GPU, in the
manner of tests/fdaf_twin.py: complex64 and float32 throughout with scipy.fft, every stage asserted to have stayed
there; wide=True is the same mathematics in complex128, the truth.  It is a yardstick for rounding, not a bit twin:
scipy's transform is not the wave-held one, an input is transformed alone and not packed with its partner, and numpy's
complex product is not the header's fmaf chain.  What it shares with the device exactly is the order of the steps, the
ring of K + 15 slots, the cut of the inputs into groups of 32 and the order of every sum, and the ramp.  A plain module:
tests/test_mconv_host.py holds it to known answers, tests/test_mconv_gpu.py measures the device against it."""
import numpy as np
import scipy.fft

F32 = np.float32
BLOCK, N, BINS = 512, 1024, 513
GROUP, ROUND = 32, 16
MAX_I, MAX_O, MAX_K, MAX_CELLS = 4096, 64, 32, 65536
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def not_finite(v):
    """gab::not_finite on the bits: the exponent all ones."""
    return (np.asarray(v, F32).view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def first_bad_tap(h):
    """(output, input, tap) of the first value of a table [n_out][n_in][L] that is not finite, or None."""
    h = np.asarray(h, F32)
    at = np.flatnonzero(not_finite(h.ravel()))
    return tuple(int(v) for v in np.unravel_index(at[0], h.shape)) if at.size else None


def tap_spectra(h, K, wide=False):
    """[...][512 K] taps in time -> [...][K][513]: partition p is the half-spectrum of [h[512 p .. 512 p + 512) | 0]."""
    real = np.float64 if wide else F32
    h = np.asarray(h, real)
    h = h.reshape(h.shape[:-1] + (K, BLOCK))
    return scipy.fft.rfft(np.concatenate([h, np.zeros_like(h)], axis=-1), axis=-1)


def groups(I):
    """The cut of the inputs: [32 g, 32 g + 32), a function of I alone."""
    return [range(lo, min(lo + GROUP, I)) for lo in range(0, I, GROUP)]


def matrix_product(Xs, H):
    """Step 2.  Xs [K][I][513]: Xs[p] is the ring slot of block b - p.  H [O][I][K][513].  Y [O][513]: per group one
    chain from zero, i ascending and inside it p ascending; then the partials in ascending g, the first as it is."""
    K, I = Xs.shape[0], Xs.shape[1]
    Y = None
    for group in groups(I):
        P = np.zeros((H.shape[0], BINS), H.dtype)
        for i in group:
            for p in range(K):
                P = P + Xs[p, i][None, :] * H[:, i, p]
        Y = P if Y is None else Y + P
    return Y


class MconvTwin:
    """The plan's state machine.  Buffers are [I][B] numpy (process) or [n][I][B] (process_batch), B a multiple of 512;
    the ramp of a ramped set runs over the next buffer given, whatever its length."""

    def __init__(self, I, O, K, wide=False):
        assert 1 <= I <= MAX_I and 1 <= O <= MAX_O and 1 <= K <= MAX_K and I * O * K <= MAX_CELLS
        self.I, self.O, self.K, self.S, self.wide = I, O, K, K + ROUND - 1, wide
        self.real, self.cplx = (np.float64, np.complex128) if wide else (F32, np.complex64)
        self.current = np.zeros((O, I, K, BINS), self.cplx)
        self.target = np.zeros((O, I, K, BINS), self.cplx)
        self.pending = False
        self.X = np.zeros((self.S, I, BINS), self.cplx)
        self.prev = np.zeros((I, BLOCK), F32)
        self.count = 0

    def set_taps(self, h, ramp=True, first_output=0, first_input=0):
        """h [n_out][n_in][512 K]; check, then commit."""
        h = np.asarray(h, F32)
        assert h.ndim == 3 and h.shape[2] == self.K * BLOCK
        assert 0 <= first_output <= self.O - h.shape[0] and 0 <= first_input <= self.I - h.shape[1]
        bad = first_bad_tap(h)
        if bad is not None:
            raise ValueError("output %d input %d tap %d" % (first_output + bad[0], first_input + bad[1], bad[2]))
        cut = (slice(first_output, first_output + h.shape[0]), slice(first_input, first_input + h.shape[1]))
        self.target[cut] = tap_spectra(h, self.K, self.wide)
        if ramp:
            self.pending = True
        else:
            self.current[cut] = self.target[cut]

    def reset(self):
        self.X[:] = 0
        self.prev[:] = 0
        self.count = 0
        self.current[:] = self.target
        self.pending = False

    def _kept(self, *arrays):
        for a in arrays:
            assert a.dtype in (self.real, self.cplx), a.dtype          # nothing was widened (or narrowed) on the way

    def _out(self, Xs, H):
        Y = matrix_product(Xs, H)
        y = scipy.fft.irfft(Y, n=N, axis=1)[:, BLOCK:] + self.real(0.0)
        self._kept(Y, y)
        return y

    def block(self, x, r=None):
        """One block: x [I][512] -> y [O][512].  r [512]: the block's piece of the ramp, on a ramp buffer."""
        b = self.count
        with np.errstate(**QUIET):
            Xn = scipy.fft.rfft(np.concatenate([self.prev, x], axis=1).astype(self.real), axis=1)
            self._kept(Xn)
            self.X[b % self.S] = Xn
            Xs = np.stack([self.X[(b - p) % self.S] for p in range(self.K)])
            y = self._out(Xs, self.target)
            if r is not None:
                yc = self._out(Xs, self.current)
                y = (y - yc) * r.astype(self.real)[None, :] + yc
                self._kept(y)
        self.prev = np.array(x, F32)
        self.count += 1
        return y

    def process(self, x):
        """x [I][B] -> [O][B]; the ramp buffer if a ramp is pending."""
        x = np.asarray(x, F32).reshape(self.I, -1)
        B = x.shape[1]
        assert B % BLOCK == 0 and B > 0
        ramp = ((np.arange(B, dtype=np.float64) + 1.0) / B).astype(F32) if self.pending else None
        out = [self.block(x[:, i:i + BLOCK], None if ramp is None else ramp[i:i + BLOCK]) for i in range(0, B, BLOCK)]
        if self.pending:
            self.current[:] = self.target
            self.pending = False
        return np.concatenate(out, axis=1)

    def process_batch(self, xs):
        """[n][I][B] -> [n][O][B]: n process calls."""
        return np.stack([self.process(x) for x in xs])

    def state(self):
        return self.current, self.target, self.X, self.prev, self.count
