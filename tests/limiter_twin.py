"""The limiter plan's contract (include/gab_c_api.h, gab_lim_*) restated in numpy; what lim_kernel must equal bit for bit.

    lim_reference   one buffer of the contract, vectorised over tracks and, outside the release, over samples.  wide=False:
                    every operation a float32 operation rounded once, fma32 (tests/test_mix_host.py) where the contract says
                    fmaf, fmin32 (tests/test_dynamics_host.py) for fminf; the detector's fmaxf runs over values that are
                    neither negative nor a NaN, where it is the plain maximum.  wide=True: the same mathematics
                    in float64 on the same float32 parameters per sample (they are the control path), the need min(1,
                    ceil / d) without the one-unit correction, which is a matter of float32 alone.
    Twin            the plan's state machine on the host: current, target, a pending ramp and the three histories [T][W-1]
                    of xd, t and e, oldest first, so a stream can be cut into buffers anywhere.  It counts the samples over
                    their ceiling and those where the correction of the quotient fired.

A plain module, no tests: tests/test_limiter_host.py holds it without trusting it, tests/test_limiter_gpu.py compares the
device against it.
"""
import numpy as np

from test_dynamics_host import fmin32
from test_mix_host import fma32, mix_ramp

f32 = np.float32
DRIVE, CEIL, REL = range(3)
FIELDS = 3
IDENTITY = np.array([1.0, 2.0 ** 32, 0.0], np.float32)       # a new plan's row: a pure delay of W - 1 samples


def sample_params(cur, tgt, ramp, B):
    """[3][T][B] float32: the target, or on a ramp buffer fmaf(target - current, r[s], current)."""
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    if ramp is None:
        return np.broadcast_to(tgt.T[:, :, None], (FIELDS, tgt.shape[0], B))
    diff = (tgt - cur).T[:, :, None]                                  # float32: one rounding
    return fma32(diff, np.asarray(ramp, np.float32)[None, None, :], cur.T[:, :, None])


def detector(xd, link):
    """d [T][B]: per link group the largest |xd| among the finite ones, from 0."""
    T, B = xd.shape
    a = np.abs(xd)
    a = np.where(a.view(np.uint32) < np.uint32(0x7f800000), a, f32(0.0)).astype(np.float32)
    return np.repeat(a.reshape(T // link, link, B).max(axis=1), link, axis=0)


def need_f32(d, c):
    """(t, over, fired): 1 where d <= c, else c / d, one unit lower where its product with d still exceeds c."""
    over = ~(d <= c)
    q = (c / np.where(over, d, f32(1.0))).astype(np.float32)          # IEEE division, one rounding
    fired = over & (q * d > c)
    q = np.where(fired, (q.view(np.uint32) - np.uint32(1)).view(np.float32), q)
    return np.where(over, q, f32(1.0)).astype(np.float32), over, fired


def window_min(tt, W):
    """The doubling form: m of every position that has W - 1 values before it, [T][len - (W - 1)]."""
    cur = tt
    h = 1
    while h < W:
        cur = np.concatenate([cur[:, :h], np.minimum(cur[:, h:], cur[:, :-h])], axis=1)
        h *= 2
    return cur[:, W - 1:]


def window_sum(ee, W):
    """S_W of the contract: S_1 = e, S_2h[n] = S_h[n] + S_h[n - h], every + rounded once in ee's dtype."""
    cur = ee
    h = 1
    while h < W:
        cur = np.concatenate([cur[:, :h], cur[:, h:] + cur[:, :-h]], axis=1)
        h *= 2
    assert cur.dtype == ee.dtype
    return cur[:, W - 1:]


def lim_reference(x, cur, tgt, ramp, hist, W, link=1, wide=False):
    """x [T][B] float32; cur / tgt [T][3]; ramp: the table [B] on a buffer with a pending ramp, else None; hist = (xd, t,
    e), each [T][W-1], oldest first.  Returns (y [T][B], gr [T], hist afterwards, g [T][B], (over, fired) counts)."""
    x = np.asarray(x, np.float32)
    T, B = x.shape
    k = W.bit_length() - 1
    assert W == 1 << k and 2 <= k <= 8
    p = sample_params(cur, tgt, ramp, B)
    dt = np.float64 if wide else np.float32
    xh, th, eh = (np.asarray(h, dt) for h in hist)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        xd32 = p[DRIVE] * x                                           # the detector's view is float32 in both forms
        if wide:
            xd = p[DRIVE].astype(np.float64) * x.astype(np.float64)
            a = np.abs(xd)
            a = np.where(np.isfinite(xd32), a, 0.0)
            d = np.repeat(a.reshape(T // link, link, B).max(axis=1), link, axis=0)
            c = p[CEIL].astype(np.float64)
            over = ~(d <= c)
            t = np.where(over, c / np.where(over, d, 1.0), 1.0)
            fired = np.zeros_like(over)
        else:
            xd = xd32
            t, over, fired = need_f32(detector(xd, link), p[CEIL])
        tt = np.concatenate([th, t], axis=1)
        m = window_min(tt, W)
        e = np.empty((T, B), dt)
        prev = eh[:, -1].copy()
        for n in range(B):
            if wide:
                r = p[REL][:, n].astype(np.float64)
                prev = np.minimum(m[:, n], r * (1.0 - prev) + prev)
            else:
                prev = fmin32(m[:, n], fma32(p[REL][:, n], f32(1.0) - prev, prev))
            e[:, n] = prev
        ee = np.concatenate([eh, e], axis=1)
        s = window_sum(ee, W) * dt(2.0 ** -k)
        xx = np.concatenate([xh, xd], axis=1)
        if wide:
            g = np.minimum(s, tt[:, :B])
            gr = g.min(axis=1)
        else:
            g = fmin32(s, tt[:, :B])
            gr = np.full(T, np.inf, np.float32)
            for n in range(B):
                gr = fmin32(gr, g[:, n])
        y = g * xx[:, :B]
    assert y.dtype == dt and g.dtype == dt
    return y, gr, (xx[:, B:], tt[:, B:], ee[:, B:]), g, (int(over.sum()), int(fired.sum()))


class Twin:
    """The plan on the host.  process(x) -> (y, gr); .g is the last buffer's gain, .over / .fired the census so far."""

    def __init__(self, T, B, W, link=1, wide=False):
        self.T, self.B, self.W, self.link, self.wide = T, B, W, link, wide
        self.latency = W - 1
        self.cur = np.tile(IDENTITY, (T, 1))
        self.tgt = self.cur.copy()
        self.pending = False
        self.over = self.fired = 0
        self._clear()

    def _clear(self):
        dt = np.float64 if self.wide else np.float32
        D = self.W - 1
        self.hist = (np.zeros((self.T, D), dt), np.ones((self.T, D), dt), np.ones((self.T, D), dt))

    def set_params(self, p, ramp=True, first_track=0):
        n = p.shape[0]
        self.tgt[first_track:first_track + n] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + n] = p

    def reset(self):
        self._clear()
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x):
        """x [T][any length]: the ramp table is that length's, as the plan's is its bufsize's."""
        B = x.shape[1]
        y, gr, self.hist, self.g, (o, f) = lim_reference(x, self.cur, self.tgt, mix_ramp(B) if self.pending else None,
                                                         self.hist, self.W, self.link, self.wide)
        self.over += o
        self.fired += f
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y, gr


def first_refused(rows):
    """The index into the flat table of the first value a set refuses (the column `admitted` of the header), or None."""
    flat = np.asarray(rows, np.float32).ravel()
    for i, v in enumerate(flat):
        field = i % FIELDS
        with np.errstate(invalid="ignore"):
            ok = ((v >= 0.0 and v <= f32(2.0 ** 32)) if field == DRIVE else
                  (v >= f32(2.0 ** -32) and v <= f32(2.0 ** 32)) if field == CEIL else (v >= 0.0 and v <= 1.0))
        if not ok:
            return i
    return None


def row(drive=1.0, ceil=1.0, rel=0.0):
    return np.array([drive, ceil, rel], np.float64).astype(np.float32)


def table(T, **kw):
    return np.tile(row(**kw), (T, 1))


def lim_mix(T, seed):
    """Rows that differ on neighbouring tracks: ceilings that the noise of `levels` exceeds often, seldom and never, fast
    and slow releases, drives above and below 1."""
    rng = np.random.RandomState(seed)
    p = np.zeros((T, FIELDS), np.float32)
    for t in range(T):
        p[t] = row(drive=(1.0, 0.5, 1.75, 1.0, 1.25)[(t + seed) % 5],
                   ceil=(0.25, 0.891, 4.0, 0.999999, 0.05, 0.5)[(t // 2 + seed) % 6] * rng.uniform(0.9, 1.1),
                   rel=(0.0, 1.0, 0.01, 0.001, 0.3)[(t // 3 + 2 * seed) % 5])
    return p


def levels(T, B, seed):
    """Noise at a level per track between -36 and +12 dB."""
    scale = np.exp2(np.random.RandomState(seed + 77).uniform(-6.0, 2.0, (T, 1)))
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)) * scale).astype(np.float32)
