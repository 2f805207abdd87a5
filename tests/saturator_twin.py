"""The saturator plan's contract restated in numpy (include/gab_c_api.h, gab_sat_*), without a GPU: two
test_resample_host.Twin around a curve stage written with that file's fma32, float32 np.where and float32 division
(SatTwin: the device's bits, state machine included), and a float64 form of a whole stream beside it
(sat_reference_f64).  A plain module: tests/test_saturator_host.py holds the restatement to known answers,
tests/test_saturator_gpu.py holds the device to the restatement."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample_host import F32, Twin as ResampleTwin, chain, default_taps, fma32, resample_taps32  # noqa: E402

CURVES = ("hard", "cubic", "rational")
LIPSCHITZ = {"hard": 1.0, "cubic": 1.5, "rational": 1.0}
FIELDS = ("drive", "bias", "level")
NEW_ROW = (1.0, 0.0, 1.0)


def curve32(x, curve):
    """S(x) in float32, every operation rounded once; comparisons, so a NaN passes through."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        if curve == "rational":
            return (x / (F32(1.0) + np.abs(x)).astype(F32)).astype(F32)
        c = np.where(x > F32(1.0), F32(1.0), np.where(x < F32(-1.0), F32(-1.0), x)).astype(F32)
        if curve == "hard":
            return c
        c2 = (c * c).astype(F32)
        return (c * fma32(F32(-0.5), c2, F32(1.5))).astype(F32)


def curve64(x, curve):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if curve == "rational":
            return x / (1.0 + np.abs(x))
        c = np.where(x > 1.0, 1.0, np.where(x < -1.0, -1.0, x))
        return c if curve == "hard" else c * (1.5 - 0.5 * c * c)


def shape32(u, drive, bias, level, curve):
    """v = level * (S(fmaf(drive, u, bias)) - S(bias)); drive, bias, level broadcast against u."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = fma32(drive, u, bias)
        d = (curve32(a, curve) - curve32(np.broadcast_to(np.asarray(bias, F32), a.shape), curve)).astype(F32)
        return (np.asarray(level, F32) * d).astype(F32)


def shape64(u, drive, bias, level, curve):
    drive, bias, level = (np.asarray(v, F32).astype(np.float64) for v in (drive, bias, level))
    with np.errstate(invalid="ignore", over="ignore"):
        return level * (curve64(drive * np.asarray(u, np.float64) + bias, curve) - curve64(bias, curve))


def ramp_table(B):
    return ((np.arange(B, dtype=np.float64) + 1.0) / float(B)).astype(F32)


def ramped_rows(current, target, B):
    """[T][3] -> [T][B][3]: base sample s takes fmaf(target - current, r[s], current) per field."""
    current, target = np.asarray(current, F32), np.asarray(target, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (target - current).astype(F32)
    return fma32(d[:, None, :], ramp_table(B)[None, :, None], current[:, None, :])


def sat_taps(oversample, up_taps=None, down_taps=None):
    """(Ku, Kd, up [R][Ku], down [1][Kd]) of a plan; the defaults are the resampler's rule, 32 and 32 R."""
    R = oversample
    Ku = default_taps(R, 1) if up_taps is None else up_taps
    Kd = default_taps(1, R) if down_taps is None else down_taps
    return Ku, Kd, resample_taps32(R, 1, Ku), resample_taps32(1, R, Kd)


def latency(oversample, Ku, Kd):
    return 0 if oversample == 1 else Ku // 2 + Kd // (2 * oversample)


def refused_row(table, first_track=0):
    """The text behind "<who>: " of the first value of table [n][3] that is not finite, or None."""
    t = np.asarray(table, F32).reshape(-1)
    bad = np.flatnonzero(~np.isfinite(t))
    if not len(bad):
        return None
    i = int(bad[0])
    return "track %d field %d (%s) must be finite; the plan keeps its parameters" % (
        first_track + i // 3, i % 3, FIELDS[i % 3])


def refused_taps(up, down, Ku, Kd):
    """The text of the first tap that is not finite, the up table before the down table, or None."""
    for name, t, K in (("up", up, Ku), ("down", down, Kd)):
        bad = np.flatnonzero(~np.isfinite(np.asarray(t, F32).reshape(-1)))
        if len(bad):
            i = int(bad[0])
            return "%s table phase %d tap %d is not finite; the plan keeps its taps" % (name, i // K, i % K)
    return None


class SatTwin:
    """The plan's state machine in float32: rows and their ramp, the two resamplers' twins, the curve between them."""

    def __init__(self, tracks, bufsize, oversample=4, curve="cubic", up_taps=None, down_taps=None):
        assert curve in CURVES and oversample in (1, 2, 4, 8)
        self.T, self.B, self.R, self.curve = tracks, bufsize, oversample, curve
        self.Ku = self.Kd = 0
        self.up = self.down = None
        if oversample > 1:
            self.Ku, self.Kd, _, _ = sat_taps(oversample, up_taps, down_taps)
            assert self.Ku % 2 == 0 and 4 <= self.Ku <= 64 and 4 <= self.Kd <= 256 and self.Kd % (2 * oversample) == 0
            self.up = ResampleTwin(tracks, bufsize, oversample, 1, K=self.Ku)
            self.down = ResampleTwin(tracks, oversample * bufsize, 1, oversample, K=self.Kd)
        self.latency = latency(oversample, self.Ku, self.Kd)
        self.current = np.tile(np.array(NEW_ROW, F32), (tracks, 1))
        self.target = self.current.copy()
        self.pending = False

    @property
    def hist_in(self):
        return self.up.hist

    @property
    def hist_os(self):
        return self.down.hist

    def reset(self):
        if self.up:
            self.up.reset()
            self.down.reset()
        self.current = self.target.copy()
        self.pending = False

    def set_params(self, table, ramp=True, first_track=0):
        table = np.array(table, F32).reshape(-1, 3)
        text = refused_row(table, first_track)
        if text:
            raise ValueError(text)
        self.target[first_track:first_track + len(table)] = table
        if ramp:
            self.pending = True
        else:
            self.current[first_track:first_track + len(table)] = table

    def set_taps(self, up, down):
        text = refused_taps(up, down, self.Ku, self.Kd)
        if text:
            raise ValueError(text)
        self.up.set_taps(up)
        self.down.set_taps(down)

    def _rows(self):
        """The rows of the next buffer, [T][B or 1][3]; a pending ramp is consumed."""
        if self.pending:
            rows = ramped_rows(self.current, self.target, self.B)
            self.current = self.target.copy()
            self.pending = False
            return rows
        return self.target[:, None, :]

    def _shape(self, u, rows):
        """u [T][R B]: all R oversampled samples of base sample s take row s."""
        r = np.repeat(rows, self.R, axis=1) if rows.shape[1] > 1 else rows
        return shape32(u, r[:, :, 0], r[:, :, 1], r[:, :, 2], self.curve)

    def apply(self, us):
        """The curve stage alone on [n][T][R B]; only the first buffer takes a pending ramp."""
        us = np.asarray(us, F32).reshape(-1, self.T, self.R * self.B)
        return np.stack([self._shape(u, self._rows()) for u in us])

    def process(self, x):
        x = np.asarray(x, F32).reshape(self.T, self.B)
        rows = self._rows()
        if self.R == 1:
            return self._shape(x, rows)
        u, n = self.up.process(x)
        assert n == self.R * self.B
        y, n = self.down.process(self._shape(u, rows))
        assert n == self.B
        return y

    def process_batch(self, xs):
        xs = np.asarray(xs, F32).reshape(-1, self.T, self.B)
        return np.stack([self.process(x) for x in xs])


def sat_reference_f64(x, row, oversample, curve, up_taps=None, down_taps=None, up=None, down=None):
    """x [T][N], a whole stream from a reset under one row {drive, bias, level}: [T][N] float64, the same float32 tables."""
    x = np.atleast_2d(np.asarray(x, F32))
    T, N = x.shape
    R = oversample
    if R == 1:
        return shape64(x, row[0], row[1], row[2], curve)
    Ku, Kd, hu, hd = sat_taps(R, up_taps, down_taps)
    hu = hu if up is None else np.asarray(up, F32).reshape(R, Ku)
    hd = hd if down is None else np.asarray(down, F32).reshape(1, Kd)
    m = np.arange(R * N, dtype=np.int64)
    u = chain(np.concatenate([np.zeros((T, Ku - 1)), x.astype(np.float64)], axis=1), hu, m // R, m % R, False)
    v = shape64(u, row[0], row[1], row[2], curve)
    m = np.arange(N, dtype=np.int64)
    return chain(np.concatenate([np.zeros((T, Kd - 1)), v], axis=1), hd, m * R, np.zeros(N, np.int64), False)
