"""The nlms plan's contract restated in numpy (include/gab_c_api.h, gab_nlms_*), without a GPU: vectorised over tracks
and taps, a Python loop over samples, every float32 operation rounded once (test_mix_host's fma32 for the fused
ones).  NlmsTwin carries the plan's two states and its ramped table through any cut into calls and batches; wide=True
does the same mathematics in float64 with plain sums.  A plain module: tests/test_nlms_host.py holds the restatement
to known answers, tests/test_nlms_gpu.py holds the device to the restatement."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_mix_host import fma32, mix_ramp  # noqa: E402

F32 = np.float32
FIELDS = ("mu", "eps")
NEW_ROW = (0.0, 1.0)
TAPS = (64, 128, 256, 512)
MU_MAX, EPS_MIN, EPS_MAX = F32(2.0), F32(2.0 ** -126), F32(2.0 ** 64)
QUIET = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def not_finite(v):
    """gab::not_finite on the bits: the exponent all ones."""
    return (np.asarray(v, F32).view(np.uint32) & np.uint32(0x7f800000)) == np.uint32(0x7f800000)


def tree32(v):
    """The balanced tree over the last axis (64 wide) in natural order, adjacent pairs first, one rounded sum each."""
    v = np.asarray(v, F32)
    assert v.shape[-1] == 64
    with np.errstate(**QUIET):
        while v.shape[-1] > 1:
            v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    return v[..., 0]


def chain32(a, b):
    """C_q per l: a, b [..., R, 64] -> [..., 64]: one rounded product, then R - 1 fmaf."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(**QUIET):
        acc = (a[..., 0, :] * b[..., 0, :]).astype(F32)
    for q in range(1, a.shape[-2]):
        acc = fma32(a[..., q, :], b[..., q, :], acc)
    return acc


def dot32(w, X):
    """y = T(C_q(w, X)) for w, X [..., L]."""
    L = w.shape[-1]
    return tree32(chain32(w.reshape(w.shape[:-1] + (L // 64, 64)), X.reshape(X.shape[:-1] + (L // 64, 64))))


def first_refused(table):
    """The flat index of the first value of a table [n][2] that the rule refuses, or None."""
    t = np.asarray(table, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        bad = not_finite(t)
        bad[:, 0] |= ~((t[:, 0] >= 0) & (t[:, 0] <= MU_MAX))
        bad[:, 1] |= ~((t[:, 1] >= EPS_MIN) & (t[:, 1] <= EPS_MAX))
    at = np.flatnonzero(bad.ravel())
    return int(at[0]) if at.size else None


def first_bad_tap(w):
    at = np.flatnonzero(not_finite(np.asarray(w, F32).ravel()))
    return int(at[0]) if at.size else None


def nlms_params(step=0.5, floor_db=-60.0, taps=64):
    """ops.nlms_params restated: {mu, eps = taps 10^(floor_db / 10)}, float64, rounded once."""
    return np.array([step, taps * 10.0 ** (floor_db / 10.0)], np.float64).astype(F32)


class NlmsTwin:
    """The plan's state machine.  Blocks are [T][B] numpy (process) or [n][T][B] (process_batch)."""

    def __init__(self, T, B, L, wide=False):
        assert L in TAPS
        self.T, self.B, self.L, self.wide = T, B, L, wide
        self.cur = np.tile(np.array(NEW_ROW, F32), (T, 1))
        self.tgt = self.cur.copy()
        self.pending = False
        self.w = np.zeros((T, L), np.float64 if wide else F32)
        self.hist = np.zeros((T, L - 1), F32)
        self.skipped = 0                  # updates left out because g was not finite

    def set_params(self, p, ramp=True, first_track=0):
        p = np.asarray(p, F32).reshape(-1, 2)
        bad = first_refused(p)
        if bad is not None:
            raise ValueError("track %d field %d" % (first_track + bad // 2, bad % 2))
        self.tgt[first_track:first_track + len(p)] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + len(p)] = p

    def set_taps(self, w, first_track=0):
        w = np.asarray(w, F32).reshape(-1, self.L)
        bad = first_bad_tap(w)
        if bad is not None:
            raise ValueError("track %d tap %d" % (first_track + bad // self.L, bad % self.L))
        self.w[first_track:first_track + len(w)] = w

    def reset(self):
        self.w[:] = 0
        self.hist[:] = 0
        self.cur[:] = self.tgt
        self.pending = False

    def sample_params(self):
        """(mu, eps), each [T][B], of the next buffer."""
        if not self.pending:
            return tuple(np.repeat(self.tgt[:, f:f + 1], self.B, axis=1) for f in (0, 1))
        r = mix_ramp(self.B)
        with np.errstate(**QUIET):
            d = (self.tgt - self.cur).astype(F32)
        return tuple(fma32(d[:, f:f + 1], r[None, :], self.cur[:, f:f + 1]) for f in (0, 1))

    def process(self, d, x):
        """d, x [T][B] -> (err, est) [T][B] float32 (float64 with wide)."""
        T, B, L = self.T, self.B, self.L
        d, x = np.asarray(d, F32).reshape(T, B), np.asarray(x, F32).reshape(T, B)
        mu, eps = self.sample_params()
        xx = np.concatenate([self.hist, x], axis=1)                   # the window of sample n: xx[:, n : n + L] reversed
        kind = np.float64 if self.wide else F32
        err, est = np.zeros((T, B), kind), np.zeros((T, B), kind)
        w = self.w
        with np.errstate(**QUIET):
            for n in range(B):
                X = xx[:, n:n + L][:, ::-1]
                if self.wide:
                    X = X.astype(np.float64)
                    y, P = (w * X).sum(axis=1), (X * X).sum(axis=1)
                    e = d[:, n].astype(np.float64) - y
                    g = mu[:, n].astype(np.float64) / (P + eps[:, n].astype(np.float64)) * e
                    ok = np.isfinite(g)
                    w = np.where(ok[:, None], w + g[:, None] * X, w)
                else:
                    both = dot32(np.stack([w, X]), np.stack([X, X]))
                    y, P = both[0], both[1]
                    e = (d[:, n] - y).astype(F32)
                    den = (P + eps[:, n]).astype(F32)
                    s = (mu[:, n] / den).astype(F32)
                    g = (s * e).astype(F32)
                    ok = ~not_finite(g)
                    w = np.where(ok[:, None], fma32(g[:, None], X, w), w)
                self.skipped += int((~ok).sum())
                err[:, n], est[:, n] = e, y
        self.w = w
        self.hist = xx[:, B:].copy()
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return err, est

    def process_batch(self, ds, xs):
        """[n][T][B] -> (err, est) [n][T][B]: n process calls (a pending ramp runs through the first)."""
        outs = [self.process(d, x) for d, x in zip(ds, xs)]
        return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])

    def copy(self):
        c = NlmsTwin(self.T, self.B, self.L, self.wide)
        c.cur, c.tgt, c.pending = self.cur.copy(), self.tgt.copy(), self.pending
        c.w, c.hist, c.skipped = self.w.copy(), self.hist.copy(), self.skipped
        return c
