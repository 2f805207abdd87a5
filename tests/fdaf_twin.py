"""The fdaf plan's contract restated in numpy (include/gab_c_api.h, gab_fdaf_*), without a GPU, in the manner of
tests/conv_pair_twin.py: complex64 and float32 throughout with scipy.fft (which keeps single precision), every stage
asserted to have stayed there; wide=True is the same mathematics in complex128, the truth.  It is a yardstick for
rounding, not a bit twin: scipy's transform is not the wave-held one, a track is transformed alone and not packed with
its partner, and numpy's complex product is not the header's fmaf chain.  What it shares with the device exactly is
the order of the steps, the ring, the skip (per PAIR of tracks), the alternated constraint and that a track whose mu
is 0 keeps its W.  A plain module:
tests/test_fdaf_host.py holds it to known answers, tests/test_fdaf_gpu.py measures the device against it."""
import numpy as np
import scipy.fft

F32 = np.float32
BLOCK, N, BINS = 512, 1024, 513
FIELDS = ("mu", "eps")
NEW_ROW = (0.0, 1.0)
MAX_K = 32
MU_MAX, EPS_MIN, EPS_MAX = F32(1.0), F32(2.0 ** -126), F32(2.0 ** 64)
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def not_finite(v):
    """gab::not_finite on the bits: the exponent all ones."""
    return (np.asarray(v, F32).view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def first_refused(table):
    """The flat index of the first value of a table [n][2] that the rule refuses, or None."""
    t = np.asarray(table, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        bad = not_finite(t)
        bad[:, 0] |= ~((t[:, 0] >= 0) & (t[:, 0] <= MU_MAX))
        bad[:, 1] |= ~((t[:, 1] >= EPS_MIN) & (t[:, 1] <= EPS_MAX))
    at = np.flatnonzero(bad.ravel())
    return int(at[0]) if at.size else None


def first_bad_tap(h):
    at = np.flatnonzero(not_finite(np.asarray(h, F32).ravel()))
    return int(at[0]) if at.size else None


def fdaf_params(step=0.5, floor_db=-60.0, partitions=1):
    """ops.fdaf_params restated: {mu, eps = partitions 1024 10^(floor_db / 10)}, float64, rounded once."""
    return np.array([step, partitions * 1024.0 * 10.0 ** (floor_db / 10.0)], np.float64).astype(F32)


def tap_spectra(h, K, wide=False):
    """[n][512 K] taps in time -> [n][K][513]: partition p is the half-spectrum of [h[512 p .. 512 p + 512) | 0]."""
    real = np.float64 if wide else F32
    h = np.asarray(h, real).reshape(-1, K, BLOCK)
    return scipy.fft.rfft(np.concatenate([h, np.zeros_like(h)], axis=-1), axis=-1)


def taps_of(W):
    """[n][K][513] -> [n][512 K]: the first 512 samples of each partition's inverse (FdafPlan.taps)."""
    return scipy.fft.irfft(W, n=N, axis=-1)[..., :BLOCK].reshape(W.shape[0], -1)


class FdafTwin:
    """The plan's state machine.  Blocks are [T][B] numpy (process) or [n][T][B] (process_batch), B a multiple of 512."""

    def __init__(self, T, K, wide=False):
        assert 1 <= K <= MAX_K
        self.T, self.K, self.wide = T, K, wide
        self.real, self.cplx = (np.float64, np.complex128) if wide else (F32, np.complex64)
        self.params = np.tile(np.array(NEW_ROW, F32), (T, 1))
        self.W = np.zeros((T, K, BINS), self.cplx)
        self.X = np.zeros((T, K, BINS), self.cplx)
        self.prev = np.zeros((T, BLOCK), F32)
        self.count = np.zeros(T, np.int64)
        self.skipped = 0                  # (pair, block)s whose steps 5 to 7 were left out

    def set_params(self, p, first_track=0):
        p = np.asarray(p, F32).reshape(-1, 2)
        bad = first_refused(p)
        if bad is not None:
            raise ValueError("track %d field %d" % (first_track + bad // 2, bad % 2))
        self.params[first_track:first_track + len(p)] = p

    def set_taps(self, h, first_track=0):
        h = np.asarray(h, F32).reshape(-1, self.K * BLOCK)
        bad = first_bad_tap(h)
        if bad is not None:
            raise ValueError("track %d tap %d" % (first_track + bad // h.shape[1], bad % h.shape[1]))
        self.W[first_track:first_track + len(h)] = tap_spectra(h, self.K, self.wide)

    def taps(self):
        return taps_of(self.W)

    def reset(self):
        for a in (self.W, self.X, self.prev, self.count):
            a[:] = 0

    def _kept(self, *arrays):
        for a in arrays:
            assert a.dtype in (self.real, self.cplx), a.dtype          # nothing was widened (or narrowed) on the way

    def block(self, d, x, adapt=True):
        """One block: d, x [T][512] -> (err, est).  adapt=False leaves steps 5 to 7 out for every pair (what a skipped
        block does), for the tests that compare against a stream without its bad blocks."""
        T, K, real = self.T, self.K, self.real
        assert (self.count == self.count[0]).all()
        slot = int(self.count[0] % K)
        mu, eps = self.params[:, 0:1].astype(real), self.params[:, 1:2].astype(real)
        with np.errstate(**QUIET):
            # 1. the window's spectrum into the ring
            Xn = scipy.fft.rfft(np.concatenate([self.prev, x], axis=1).astype(real), axis=1)
            self.X[:, slot] = Xn
            # 2. Y and S, p ascending
            order = [(slot - p) % K for p in range(K)]
            Y = np.zeros((T, BINS), self.cplx)
            S = np.zeros((T, BINS), real)
            for p, sp in enumerate(order):
                Xp = self.X[:, sp]
                Y = Y + Xp * self.W[:, p]
                S = S + (Xp.real * Xp.real + Xp.imag * Xp.imag)
            self._kept(Xn, Y, S)
            # 3. the estimate and the error
            est = scipy.fft.irfft(Y, n=N, axis=1)[:, BLOCK:] + real(0.0)
            err = d.astype(real) - est
            self._kept(est, err)
            # 4. the skip, per pair
            bad = ~np.isfinite(err).all(axis=1)
            bad = np.repeat(np.logical_or.reduceat(bad, np.arange(0, T, 2)), 2)[:T]
            if not adapt:
                bad[:] = True
            self.skipped += int(bad[0::2].sum())
            # 5. to 7.
            E = scipy.fft.rfft(np.concatenate([np.zeros_like(err), err], axis=1), axis=1)
            G = (mu / (S + eps)) * E
            Wn = self.W.copy()
            for p, sp in enumerate(order):
                Wn[:, p] = Wn[:, p] + np.conj(self.X[:, sp]) * G
            w = scipy.fft.irfft(Wn[:, slot], n=N, axis=1)
            w[:, BLOCK:] = 0
            Wn[:, slot] = scipy.fft.rfft(w, axis=1)
            self._kept(E, G, Wn, w)
            keep = bad | (self.params[:, 0] == 0)                        # a track with mu = 0 never writes its W
            self.W = np.where(keep[:, None, None], self.W, Wn)
        self.prev = np.array(x, F32)
        self.count += 1
        return err, est

    def process(self, d, x, adapt=True):
        """d, x [T][B] -> (err, est) [T][B]."""
        d, x = np.asarray(d, F32).reshape(self.T, -1), np.asarray(x, F32).reshape(self.T, -1)
        assert d.shape == x.shape and d.shape[1] % BLOCK == 0 and d.shape[1] > 0
        outs = [self.block(d[:, i:i + BLOCK], x[:, i:i + BLOCK], adapt) for i in range(0, d.shape[1], BLOCK)]
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)

    def process_batch(self, ds, xs):
        """[n][T][B] -> (err, est) [n][T][B]: n process calls."""
        outs = [self.process(d, x) for d, x in zip(ds, xs)]
        return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])

    def state(self):
        return self.W, self.X, self.prev, self.count
