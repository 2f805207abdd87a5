"""The gate plan (gab_gate_*) without a GPU: the restatement the GPU tests compare against, held without trusting it.

    gate_reference_f32  the contract of include/gab_c_api.h in numpy, vectorised over tracks and, outside the state
                        machine and the glide, over samples: every operation a float32 operation rounded once, fma32
                        (tests/test_mix_host.py) where the contract says fmaf, fmax32 (tests/test_dynamics_host.py) for
                        the detector.  What gate_kernel must equal bit for bit.
    gate_reference_f64  its twin: the same float32 parameters per sample and the same decisions (the detector, the two
                        comparisons and the count work on float32 data and integers: they are exact, and the gain never
                        enters them), the glide g = tg + al (g - tg) in float64.

The a-priori bound of |g32 - g64| (gate_bound), u = 2^-24, for gains within [0, Gmax] and att, rel <= A: both sides take
the same al and tg at every sample, so an error e of g passes as al e; the float32 side adds its own two roundings per
step, g - tg (at most u Gmax, and multiplied by al <= 1) and the fmaf (at most u Gmax), which the recurrence keeps within
                                                                                    bound = 2 u Gmax / (1 - A)
Derived as the dynamics plan's is, not measured; the figures of every case: pytest -s.

Without the feature every test here fails at the import of GatePlan / gate_params or at a gab_gate_* symbol, and every
test of tests/test_gate_gpu.py.
"""
import ctypes
import math

import numpy as np
import pytest

from plan_helpers import bits
from test_dynamics_host import fmax32
from test_mix_host import EPS, fma32, mix_ramp

f32 = np.float32
IDENTITY = np.array([0, 0, 0, 0, 1, 1, 0], np.float32)
OPEN, CLOSE, ATT, REL, G_OPEN, G_CLOSED, HOLD = range(7)
CAP = f32(1.0 - 2.0 ** -20)


def detector(k, link):
    """a [T][B]: |k| from 0 with NaN ignored, the maximum over each link group."""
    T, B = k.shape
    a = fmax32(f32(0.0), np.abs(k))
    return np.repeat(a.reshape(T // link, link, B).max(axis=1), link, axis=0)


def sample_params(cur, tgt, ramp, B):
    """[7][T][B] float32: the target, or on a ramp buffer fmaf(target - current, r[s], current) for fields 0 to 5 and
    the target's hold."""
    cur, tgt = np.asarray(cur, np.float32), np.asarray(tgt, np.float32)
    if ramp is None:
        return np.broadcast_to(tgt.T[:, :, None], (7, tgt.shape[0], B))
    diff = (tgt - cur).T[:, :, None]                                  # float32: one rounding
    p = fma32(diff, np.asarray(ramp, np.float32)[None, None, :], cur.T[:, :, None])
    p[HOLD] = tgt[:, HOLD, None]
    return p


def _run(x, key, cur, tgt, ramp, g, c, link, wide):
    """-> (y [T][B], act [T] int32, g [T], c [T] int32, G [T][B]: the gain per sample, O [T][B]: open or not)"""
    x = np.asarray(x, np.float32)
    T, B = x.shape
    k = x if key is None else np.asarray(key, np.float32)
    p = sample_params(cur, tgt, ramp, B)
    H = np.asarray(tgt, np.float32)[:, HOLD].astype(np.int32)
    a = detector(k, link)
    above, between = a > p[OPEN], a >= p[CLOSE]                       # float32 comparisons: exact
    G = np.empty((T, B), np.float64 if wide else np.float32)
    O = np.empty((T, B), bool)
    g = np.array(g, G.dtype)
    c = np.array(c, np.int32)
    for n in range(B):
        held = np.where(c >= 0, H, -1)
        down = np.maximum(c - 1, -1)
        c = np.where(above[:, n], H, np.where(between[:, n], held, down)).astype(np.int32)
        o = c >= 0
        tg = np.where(o, p[G_OPEN][:, n], p[G_CLOSED][:, n])
        al = np.where(o, p[ATT][:, n], p[REL][:, n])
        if wide:
            g = al.astype(np.float64) * (g - tg) + tg
        else:
            g = fma32(al, g - tg, tg)
        G[:, n] = g
        O[:, n] = o
    with np.errstate(invalid="ignore", over="ignore"):
        y = x.astype(G.dtype) * G
    return y, O.sum(axis=1).astype(np.int32), g, c, G, O


def gate_reference_f32(x, key, cur, tgt, ramp, g, c, link=1):
    """x, key [T][B] float32 (key may be None), cur / tgt [T][7] float32; ramp: the table [B] on a buffer with a pending
    ramp, else None; g [T] float32 and c [T] int32: the carried gain and count.  Returns (y [T][B] float32, act [T]
    int32, g afterwards, c afterwards)."""
    y, act, g, c, _, _ = _run(x, key, cur, tgt, ramp, g, c, link, False)
    assert y.dtype == np.float32 and g.dtype == np.float32 and c.dtype == np.int32 and act.dtype == np.int32
    return y, act, g, c


def gate_reference_f64(x, key, cur, tgt, ramp, g, c, link=1):
    y, act, g, c, _, _ = _run(x, key, cur, tgt, ramp, g, c, link, True)
    return y, act, g, c


def gate_bound(Gmax, A):
    """The bound on |g32 - g64| of the module's docstring."""
    return 2.0 * EPS * Gmax / (1.0 - A)


def gate_first_refused(table):
    """The host twin of the device rule: the index into the flat table of the first value outside the contract, or None."""
    t = np.asarray(table, np.float32).reshape(-1, 7)
    for i, v in enumerate(t.ravel()):
        field = i % 7
        bad = not np.isfinite(v) or not v >= 0.0
        if field == OPEN:
            bad = bad or not v <= f32(2.0 ** 64)
        if field == CLOSE:
            bad = bad or not v <= t.ravel()[i - 1]
        if field in (ATT, REL):
            bad = bad or not v <= CAP
        if field in (G_OPEN, G_CLOSED):
            bad = bad or not v <= 256.0
        if field == HOLD:
            bad = bad or not v <= 2.0 ** 24 or np.trunc(v) != v
        if bad:
            return i
    return None


class Twin:
    """The plan's state machine on the host: current, target, a pending ramp, the gain and the count; process() is
    gate_reference_f32."""

    def __init__(self, T, B, link=1):
        self.T, self.B, self.link = T, B, link
        self.cur = np.tile(IDENTITY, (T, 1))
        self.tgt = self.cur.copy()
        self.pending = False
        self.g = np.ones(T, np.float32)
        self.c = np.full(T, -1, np.int32)

    def set_params(self, p, ramp=True, first_track=0):
        assert gate_first_refused(p) is None
        n = p.shape[0]
        self.tgt[first_track:first_track + n] = p
        if ramp:
            self.pending = True
        else:
            self.cur[first_track:first_track + n] = p

    def reset(self):
        self.g = self.tgt[:, G_CLOSED].copy()
        self.c = np.full(self.T, -1, np.int32)
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x, key=None):
        y, act, self.g, self.c = gate_reference_f32(x, key, self.cur, self.tgt, mix_ramp(self.B) if self.pending else None,
                                                    self.g, self.c, self.link)
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y, act


def row(open=0.0, close=None, att=0.0, rel=0.0, g_open=1.0, g_closed=0.0, hold=0):
    return np.array([open, open if close is None else close, att, rel, g_open, g_closed, hold], np.float64).astype(np.float32)


def table(T, **kw):
    return np.tile(row(**kw), (T, 1))


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def gate_mix(T, seed):
    """Parameter rows that differ on neighbouring tracks: gates and duckers, with and without hysteresis, holds of 0, a
    few samples and longer than a buffer, fast and slow glides, a floor of 0 on some.  Thresholds around the levels of
    `bursts`."""
    rng = np.random.RandomState(seed)
    p = np.zeros((T, 7), np.float32)
    for t in range(T):
        op = rng.uniform(0.05, 0.6)
        duck = (t + seed) % 4 == 3
        p[t] = row(open=op, close=op * (1.0, 0.7, 0.3, 0.0)[(t + seed) % 4], att=(0.0, 0.5, 0.9, 0.99)[(t // 2 + seed) % 4],
                   rel=(0.999, 0.9, 0.0, 0.97, 0.5)[(t // 3 + seed) % 5], g_open=rng.uniform(0.1, 0.5) if duck else (1.0, 2.0)[t % 2],
                   g_closed=1.0 if duck else (0.0, 0.1, 0.0)[(t + seed) % 3], hold=(0, 3, 40, 700, 1)[(t + 2 * seed) % 5])
    return p


def bursts(T, B, seed):
    """Noise whose level per track moves in steps of a few dozen samples between silence, around the thresholds of
    gate_mix and full scale: gates open, hold, close and re-open inside a buffer."""
    rng = np.random.RandomState(seed + 77)
    steps = (B + 15) // 16
    level = rng.choice([0.0, 0.02, 0.2, 0.5, 1.0], size=(T, steps))
    return (noise(T, B, seed) * np.repeat(level, 16, axis=1)[:, :B]).astype(np.float32)


def closed(T, g=0.0):
    return np.full(T, g, np.float32), np.full(T, -1, np.int32)


# ---- known answers ----------------------------------------------------------------------------------------------
def test_a_new_plans_table_is_the_identity():
    T, B = 4, 300
    x = (noise(T, B, 1).astype(np.float64) * np.exp(np.random.RandomState(2).uniform(-80, 80, (T, B)))).astype(np.float32)
    x[0, 5], x[1, 7], x[2, 0], x[3, 299], x[3, 4] = np.inf, -np.inf, 0.0, -0.0, np.nan
    p = np.tile(IDENTITY, (T, 1))
    for link in (1, 2, 4):
        for ramp in (None, mix_ramp(B)):
            y, act, g, c = gate_reference_f32(x, None, p, p, ramp, np.ones(T, np.float32), np.full(T, -1, np.int32), link)
            assert np.array_equal(bits(y), bits(x))                   # (numpy's x * 1 keeps a NaN's payload)
            assert (g == 1.0).all()


def test_the_gate_opens_on_the_first_sample_above_open_and_not_before():
    p = table(1, open=0.5, close=0.25, g_open=1.0, g_closed=0.0)
    half, above = f32(0.5), np.nextafter(f32(0.5), f32(1.0))
    x = np.array([[0.1, 0.4, half, -half, above, 0.0]], np.float32)
    y, act, g, c, G, O = _run(x, None, p, p, None, *closed(1), 1, False)
    assert O[0].tolist() == [False, False, False, False, True, False]    # a == open does not open; hold 0 shuts at once
    assert np.array_equal(y[0], np.array([0, 0, 0, 0, above, 0], np.float32)) and act[0] == 1 and c[0] == -1
    x[0, 4] = -above                                                  # the detector is |x|
    assert _run(x, None, p, p, None, *closed(1), 1, False)[5][0, 4]


@pytest.mark.parametrize("hold", [0, 1, 5, 40])
def test_the_gate_is_open_for_exactly_hold_samples_below_close(hold):
    """Buffers of 16 samples: hold = 40 is longer than a buffer, so the count is carried across them."""
    B, n = 16, 5
    p = table(1, open=0.5, close=0.25, hold=hold)
    x = np.zeros((1, B * n), np.float32)
    x[0, 3] = 1.0                                                     # one sample above open, then silence
    g, c = closed(1)
    open_at = []
    for k in range(n):
        _, act, g, c, _, O = _run(x[:, k * B:(k + 1) * B], None, p, p, None, g, c, 1, False)
        open_at += (k * B + np.flatnonzero(O[0])).tolist()
        assert act[0] == O[0].sum()
    assert open_at == list(range(3, 3 + 1 + hold))                    # the sample itself and `hold` more
    assert c[0] == -1


def test_a_level_between_the_thresholds_keeps_the_state_and_rearms_the_hold():
    p = table(1, open=0.5, close=0.25, hold=2)
    mid = np.full((1, 50), 0.3, np.float32)
    _, act, g, c, _, O = _run(mid, None, p, p, None, *closed(1), 1, False)
    assert not O.any() and c[0] == -1 and act[0] == 0                 # does not open a closed gate
    x = mid.copy()
    x[0, 0] = 0.9
    _, act, g, c, _, O = _run(x, None, p, p, None, *closed(1), 1, False)
    assert O.all() and c[0] == 2 and act[0] == 50                     # holds an open one, the count re-armed every sample
    x[0, 10:12] = 0.0                                                 # two samples below close: the hold of 2 bridges them
    assert _run(x, None, p, p, None, *closed(1), 1, False)[5].all()
    x[0, 10:13] = 0.0                                                 # three do not, and 0.3 does not open it again
    O = _run(x, None, p, p, None, *closed(1), 1, False)[5][0]
    assert O[:12].all() and not O[12:].any()


@pytest.mark.parametrize("which", ["attack", "release"])
def test_time_constants(which):
    """After ms fs / 1000 samples the gain has covered 1 - 1/e of its way: within the float32 bound and the rounding of
    the coefficient itself (a relative u of a coefficient moves its N-th power by at most N u)."""
    from gpuaudiobench_amd import gate_params
    ms, fs = 2.0, 48000.0
    N = int(ms * fs / 1000.0)
    p = gate_params(-20.0, attack_ms=ms, release_ms=ms, hold_ms=0.0, fs=fs)[None, :]
    loud, quiet = np.full((1, N), 1.0, np.float32), np.zeros((1, N), np.float32)
    if which == "attack":
        _, _, g, _ = gate_reference_f32(loud, None, p, p, None, *closed(1))
        covered = float(g[0])
    else:
        _, _, g, _ = gate_reference_f32(quiet, None, p, p, None, np.ones(1, np.float32), np.full(1, -1, np.int32))
        covered = 1.0 - float(g[0])
    tol = gate_bound(1.0, float(p[0, ATT])) + N * EPS
    print("%s: covered %.9f, 1 - 1/e %.9f, tolerance %.3g" % (which, covered, 1.0 - math.exp(-1.0), tol))
    assert abs(covered - (1.0 - math.exp(-1.0))) <= tol


def test_the_ducker_row_lowers_the_track_while_the_key_is_loud_and_restores_it():
    from gpuaudiobench_amd import gate_params
    p = gate_params(-20.0, attack_ms=0.5, release_ms=0.5, hold_ms=0.0, duck_db=-12.0)[None, :]
    assert p[0, G_CLOSED] == 1.0 and p[0, G_OPEN] == f32(10.0 ** (-12.0 / 20.0))
    B = 2000
    x = np.full((1, B), 0.5, np.float32)
    key = np.zeros((1, B), np.float32)
    key[0, 500:1000] = 0.8
    y, act, g, c, G, O = _run(x, key, p, p, None, np.ones(1, np.float32), np.full(1, -1, np.int32), 1, False)
    assert (y[0, :500] == 0.5).all() and act[0] == 500
    assert abs(float(G[0, 999]) - float(p[0, G_OPEN])) < 1e-6        # 20 time constants in: ducked by 12 dB
    assert (np.diff(G[0, 500:1000]) <= 0).all() and (np.diff(G[0, 1000:]) >= 0).all()
    assert abs(float(y[0, -1]) - 0.5) < 1e-6                          # and restored
    # without the key the track's own level (0.5, above open) would hold it ducked throughout
    assert _run(x, None, p, p, None, np.ones(1, np.float32), np.full(1, -1, np.int32), 1, False)[5].all()


def test_hysteresis_and_hold_toggle_less_than_a_bare_threshold():
    n = np.arange(9600)
    x = (0.25 * (1.0 + np.sin(2 * np.pi * 5.0 * n / 48000.0)) + 0.02 * np.random.RandomState(3).standard_normal(n.size))
    x = x.astype(np.float32)[None, :]                                  # a slow swell through 0.25, with noise on it

    def toggles(p):
        O = _run(x, None, p, p, None, *closed(1), 1, False)[5][0]
        return int(np.count_nonzero(O[1:] != O[:-1]))
    bare = toggles(table(1, open=0.25, close=0.25, hold=0))
    calm = toggles(table(1, open=0.25, close=0.18, hold=48))
    print("toggles: bare threshold %d, with hysteresis and hold %d" % (bare, calm))
    assert calm >= 1 and bare > 4 * calm


def test_linked_tracks_share_the_detector_and_keep_their_rows():
    p = np.stack([row(open=0.5, close=0.5), row(open=0.05, close=0.05), row(open=0.5, close=0.5), row(open=0.5, close=0.5)])
    x = np.stack([np.full(20, 0.1, np.float32), np.full(20, 0.9, np.float32), np.full(20, 0.1, np.float32),
                  np.full(20, 0.2, np.float32)])
    O = _run(x, None, p, p, None, *closed(4), 2, False)[5]
    assert O[0].all() and O[1].all() and not O[2].any() and not O[3].any()       # track 0 opens on track 1's level
    O = _run(x, None, p, p, None, *closed(4), 1, False)[5]
    assert not O[0].any() and O[1].all()


def test_the_buffer_behind_a_ramp_buffer_is_steady():
    T, B = 6, 48
    p0, p1 = gate_mix(T, 1), gate_mix(T, 2)
    twin = Twin(T, B)
    twin.set_params(p0, ramp=False)
    twin.process(bursts(T, B, 1))
    twin.set_params(p1)
    x1, x2 = bursts(T, B, 2), bursts(T, B, 3)
    y1, _ = twin.process(x1)
    assert not twin.pending and np.array_equal(twin.cur, p1)
    g, c = twin.g.copy(), twin.c.copy()
    y2, act2 = twin.process(x2)
    want, want_act, _, _ = gate_reference_f32(x2, None, p1, p1, None, g, c)
    assert np.array_equal(bits(y2), bits(want)) and np.array_equal(act2, want_act)
    # the ramp's last sample takes the target itself (r = 1: current + (target - current) is exact or rounds to it) ...
    last = sample_params(p0, p1, mix_ramp(B), B)[:, :, -1].T
    assert np.abs(last[:, :6].astype(np.float64) - p1[:, :6]).max() <= 2 * EPS * 2.0
    # ... and the hold is the target's from the first
    assert np.array_equal(sample_params(p0, p1, mix_ramp(B), B)[HOLD][:, 0], p1[:, HOLD])


def test_resuming_from_copied_state_is_bit_identical_to_running_through():
    T, B = 8, 200
    p = gate_mix(T, 4)
    x = bursts(T, B, 5)
    y, act, g, c = gate_reference_f32(x, None, p, p, None, *closed(T))
    ya, acta, ga, ca = gate_reference_f32(x[:, :77], None, p, p, None, *closed(T))
    yb, actb, gb, cb = gate_reference_f32(x[:, 77:], None, p, p, None, ga.copy(), ca.copy())
    assert np.array_equal(bits(np.concatenate([ya, yb], axis=1)), bits(y))
    assert np.array_equal(bits(gb), bits(g)) and np.array_equal(cb, c) and np.array_equal(acta + actb, act)
    assert (act > 0).any() and (act < B).any() and (c >= 0).any()


def test_nonfinite_samples_reach_the_output_and_nothing_else():
    T, B = 2, 64
    p = table(T, open=0.3, close=0.1, att=0.5, rel=0.9, hold=3)
    x = bursts(T, B, 6)
    clean = _run(x, None, p, p, None, *closed(T), 1, False)
    x2 = x.copy()
    x2[0, 20], x2[1, 30] = np.inf, -np.inf                            # an infinity is a loud sample: it may open the gate
    y, act, g, c, G, O = _run(x2, None, p, p, None, *closed(T), 1, False)
    assert np.isfinite(G).all() and O[0, 20] and O[1, 30]
    x3 = x.copy()
    x3[0, 10] = np.nan                                                # a NaN reads as silence
    x0 = x.copy()
    x0[0, 10] = 0.0
    got, want = _run(x3, None, p, p, None, *closed(T), 1, False), _run(x0, None, p, p, None, *closed(T), 1, False)
    assert np.array_equal(bits(got[4]), bits(want[4])) and np.array_equal(got[3], want[3])
    assert np.isnan(got[0][0, 10]) and np.isfinite(np.delete(got[0][0], 10)).all()
    # in the key: a NaN is ignored, an infinity opens the gate, neither reaches the output
    key = np.zeros((T, B), np.float32)
    key[0, 5], key[1, 7] = np.nan, np.inf
    y, act, g, c, G, O = _run(x, key, p, p, None, *closed(T), 1, False)
    assert np.isfinite(y).all() and not O[0].any() and O[1, 7:11].all() and not O[1, :7].any() and not O[1, 11:].any()
    assert clean[1].sum() > 0


def test_the_rule_names_the_first_refused_index():
    up = lambda v: np.nextafter(f32(v), f32(np.inf))                   # noqa: E731
    good = gate_mix(5, 1)
    assert gate_first_refused(good) is None and gate_first_refused(np.tile(IDENTITY, (3, 1))) is None
    edge = np.array([[2.0 ** 64, 2.0 ** 64, CAP, CAP, 256, 256, 2.0 ** 24], [0, -0.0, 0, 0, 0, 0, -0.0]], np.float32)
    assert gate_first_refused(edge) is None
    cases = [((0, OPEN), np.nan), ((1, OPEN), up(2.0 ** 64)), ((2, OPEN), -1e-30), ((3, OPEN), np.inf),
             ((1, CLOSE), up(good[1, OPEN])), ((2, CLOSE), -1e-30), ((0, ATT), up(CAP)), ((4, ATT), -1e-30),
             ((3, REL), 1.0), ((2, REL), np.nan), ((1, G_OPEN), up(256.0)), ((0, G_OPEN), -1e-30), ((4, G_CLOSED), np.inf),
             ((2, HOLD), 2.5), ((3, HOLD), up(2.0 ** 24)), ((0, HOLD), -1.0), ((1, HOLD), np.nan)]
    assert {w[1] for w, _ in cases} == set(range(7))
    for where, value in cases:
        bad = good.copy()
        bad[where] = value
        if where[0] + 1 < 5:
            bad[where[0] + 1, G_OPEN] = np.nan                        # the FIRST offender is named
        assert gate_first_refused(bad) == where[0] * 7 + where[1], (where, value)
    # lowering open below close is named at close, the value that is held against its neighbour
    bad = good.copy()
    bad[2, OPEN] = good[2, CLOSE] * f32(0.5) if good[2, CLOSE] > 0 else f32(0.0)
    bad[2, CLOSE] = max(good[2, CLOSE], f32(0.01))
    assert gate_first_refused(bad) == 2 * 7 + CLOSE


def test_gate_params():
    from gpuaudiobench_amd import gate_params
    r = gate_params(-30.0, close_db=-36.0, attack_ms=0.5, release_ms=80.0, hold_ms=20.0, range_db=-40.0, fs=48000.0)
    assert r.shape == (7,) and r.dtype == np.float32
    want = [10.0 ** (-30.0 / 20.0), 10.0 ** (-36.0 / 20.0), math.exp(-1.0 / 24.0), math.exp(-1.0 / 3840.0), 1.0,
            10.0 ** (-40.0 / 20.0), 960.0]
    assert np.array_equal(r, np.array(want, np.float64).astype(np.float32))
    r = gate_params(-30.0, attack_ms=0.0, release_ms=0.0, hold_ms=0.0)
    want = [10.0 ** (-30.0 / 20.0), 10.0 ** (-33.0 / 20.0), 0.0, 0.0, 1.0, 0.0, 0.0]
    assert np.array_equal(r, np.array(want, np.float64).astype(np.float32))
    r = gate_params(-24.0, duck_db=-9.0)
    assert r[G_OPEN] == f32(10.0 ** (-9.0 / 20.0)) and r[G_CLOSED] == 1.0
    t = gate_params([-10.0, -20.0, -30.0], hold_ms=[0.0, 1.0, 2.0], fs=44100.0)
    assert t.shape == (3, 7) and t[:, HOLD].tolist() == [0.0, 44.0, 88.0] and (t[:, CLOSE] < t[:, OPEN]).all()
    assert gate_params(0.0, attack_ms=1e9, release_ms=1e9)[ATT] == CAP and gate_params(0.0, hold_ms=1e9)[HOLD] == 2.0 ** 24
    assert gate_first_refused(t) is None and gate_first_refused(r) is None
    for bad in (dict(open_db=-20.0, close_db=-10.0), dict(open_db=0.0, attack_ms=-1.0), dict(open_db=0.0, hold_ms=-1.0),
                dict(open_db=0.0, range_db=3.0), dict(open_db=0.0, duck_db=3.0), dict(open_db=0.0, range_db=-3.0, duck_db=-3.0)):
        with pytest.raises(ValueError):
            gate_params(**bad)


# ---- float32 against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [1, 2])
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("ramp", [False, True])
def test_float32_is_within_its_bound_of_float64(link, keyed, ramp):
    T, B, n = 16, 64, 12
    A, Gmax = 0.999, 2.0
    rng = np.random.RandomState(11 + link + 2 * keyed)

    def rows():
        p = gate_mix(T, int(rng.randint(100)))
        p[:, ATT], p[:, REL] = rng.uniform(0.0, A, T), rng.uniform(0.9, A, T)
        p[0, ATT], p[1, REL] = A, A
        return p.astype(np.float32)

    tables = [rows(), rows()]
    assert max(t[:, [G_OPEN, G_CLOSED]].max() for t in tables) <= Gmax
    cur = tgt = tables[0]
    g32, c32 = closed(T)
    g64, c64 = g32.astype(np.float64), c32.copy()
    worst, opened = 0.0, 0
    for k in range(n):
        x = bursts(T, B, 300 + k)
        key = bursts(T, B, 400 + k) if keyed else None
        r = None
        if ramp and k % 3 == 1:
            tgt = tables[(k // 3 + 1) % 2]
            r = mix_ramp(B)
        _, act, g32, c32, G32, _ = _run(x, key, cur, tgt, r, g32, c32, link, False)
        _, act64, g64, c64, G64, _ = _run(x, key, cur, tgt, r, g64, c64, link, True)
        assert np.array_equal(c32, c64) and np.array_equal(act, act64)        # the decisions are shared
        worst = max(worst, float(np.abs(G32.astype(np.float64) - G64).max()))
        opened += int(act.sum())
        if r is not None:
            cur = tgt
    bound = gate_bound(Gmax, A + EPS)                                 # (a ramped coefficient may land 2^-24 above A)
    print("link %d, %s, %s: |g32 - g64| %.3g, bound %.3g (err / bound %.3g); %d open samples"
          % (link, "keyed" if keyed else "own input", "ramps" if ramp else "steady", worst, bound, worst / bound, opened))
    assert 0 < opened < n * T * B
    assert bound <= 2.5e-4                                            # the bound itself means something: -72 dB of full scale
    assert worst <= bound


# ---- the library without a GPU --------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    """What is refused before any device call: null pointers, a bad link, tracks % link != 0.  (A track range outside the
    plan is refused the same way, but needs a plan to be outside of: tests/test_gate_gpu.py.)"""
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 1), (-1, 512, 1), (4, 0, 1), (4, -5, 1), (4, 512, 0), (4, 512, -2), (4, 512, 3), (6, 512, 4),
                 (128, 512, 128), (64, 512, 48), (3, 512, 2)):
        assert lib.gab_gate_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_gate_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_gate_create(None, 4, 512, 1) == bad
    assert b"gab_gate_create" in lib.gab_last_error() and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_gate_process(None, None, None, None, None, None), b"gab_gate_process"),
                       (lambda: lib.gab_gate_process_batch(None, None, None, None, None, 1, None), b"gab_gate_process_batch"),
                       (lambda: lib.gab_gate_set_params(None, None, 1, None), b"gab_gate_set_params"),
                       (lambda: lib.gab_gate_set_params_tracks(None, None, 0, 1, 1, None), b"gab_gate_set_params_tracks"),
                       (lambda: lib.gab_gate_params(None, None, None, None), b"gab_gate_params"),
                       (lambda: lib.gab_gate_state(None, None, None, None), b"gab_gate_state"),
                       (lambda: lib.gab_gate_reset(None, None), b"gab_gate_reset"),
                       (lambda: lib.gab_gate_destroy(None), b"gab_gate_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_gate_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_gate_create(C.byref(h), 4, 512, 2)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_gate_create" in text


def test_gate_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "GatePlan" in g.__all__ and "gate_params" in g.__all__
    assert callable(g.GatePlan) and callable(g.gate_params)
    for name in ("set_params", "reset", "process", "process_batch", "params", "state", "prepare", "launch", "close"):
        assert hasattr(g.GatePlan, name), name
    assert len(g.GatePlan.FIELDS) == 7 and g.GatePlan.FIELDS == ("open", "close", "att", "rel", "g_open", "g_closed", "hold")
