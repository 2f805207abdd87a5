"""Eight bit-exact plans (mix, delay, meter, resample, dynamics, reverb, limiter, crossover) at the edges of float32,
without a GPU: the yardstick is shown to be exact there, and the cases are shown to reach the edge.

    1. numpy keeps subnormals in this process (nothing below means anything if it flushes).
    2. every fma32 the twins use (tests/test_mix_host.py, and the wrappers of test_meter_host.py, test_resample_host.py
       and test_reverb_host.py around it) against exact rational arithmetic (round32_exact): products that underflow,
       subnormal results, ties at the subnormal spacing, underflow to a signed zero, exact cancellations, the two sides of
       the overflow boundary, a product that overflows alone but not with its addend, operands that are not finite.
    3. CASES, the one table both this file and tests/test_edges_gpu.py build their inputs from.  A case is played once
       through the plan's float32 twin (reference()): the tape of calls it records is what the device test replays.  The
       counts of what a regime is named for (subnormal outputs, subnormal state words at the end, +inf, -inf, NaN, -0.0)
       are pinned in the table; `pytest -s` prints them.  They are conditions on the reference alone.

The regimes:
    tail     one buffer of noise, then silence until the twin's carried state is subnormal or zero everywhere (a cap on
             the buffer count fails the case if the tail does not die).  Mix and resample carry nothing that decays:
             their inputs and gains are scaled so that the products are subnormal.  Dynamics: the smoothed gain runs from
             a few units up to -0 through the negative subnormals.
    quiet    dynamics only: noise at 2^-120 under gain reduction, the detector on its 2^-96 floor.
    flt_max  noise at 2^126 or 2^127: some samples overflow, their neighbours do not; an inf - inf in the loops; then
             ordinary buffers while the damage lasts, a reset, and a buffer that must be finite again.  Limiter: drives
             above 1, so that xd = drive x overflows, and every ceiling on a ramp from one end of its admitted range to
             the other (2^-32, 2^32); a need of 2^-32 / 2^127 is zero, and zero times an infinite xd a NaN.  Its finite
             outputs stay at or below the ceiling, so no finite value above 2^127 stands beside its infinities.
             Crossover: splits at 20 Hz and at 23 kHz; the integrators overflow, inf - inf follows, and the NaN stays
             in the state (a set keeps it) until the reset.
    zeros    blocks of +0.0, of -0.0 and of both, on a steady buffer, a ramp buffer and the buffer behind a ramp buffer;
             tables with negative values and -0.0 (rows that do not move keep their -0.0 across a ramp, which is where
             fmaf(+0, r, -0.0) = +0.0 shows).  Crossover: no ramp; the blocks stand on the buffers behind each set.
    contain  mix and delay: a NaN in track 64 and an infinity in the last track of buffer 1, beside the same case clean.

A mix plan cannot produce a -0.0 (a leaf's chain starts from +0.0, and +0 + -0 is +0), and a meter's rows cannot either
(every field is a magnitude, a sum from +0 or a flag): their -0.0 count is pinned at 0 for that reason."""
import collections
import functools
import types
from fractions import Fraction

import numpy as np
import pytest
import torch  # noqa: F401  (the first test is about numpy AFTER this import)

import test_meter_host
import test_mix_host
import test_resample_host
import test_reverb_host
from plan_helpers import bits
from strip_helpers import OUTPUTS, HostStrip, same, scenario, schedule
import limiter_twin
import spectrum_twin
from test_crossover_host import Twin as XoverTwin
from test_crossover_host import rows32 as xover_rows32
from test_crossover_host import xover_first_refused
from test_delay_host import Twin as DelayTwin
from test_delay_host import capacity as delay_capacity
from test_delay_host import delay_mix
from test_dynamics_host import Twin as DynTwin
from test_dynamics_host import dyn_mix
from test_gate_host import Twin as GateTwin
from test_gate_host import gate_first_refused
from test_meter_host import Twin as MeterTwin
from test_mix_host import Twin as MixTwin
from test_mix_host import gains, round32_exact
from test_resample_host import Twin as ResampleTwin
from test_reverb_host import MIN_DELAY as REVERB_MIN_DELAY
from test_reverb_host import Twin as ReverbTwin
from test_reverb_host import first_refused_param as reverb_first_refused
from test_reverb_host import reverb_mix

f32 = np.float32
TINY = f32(2.0 ** -126)                       # the smallest normal float32
FLT_MAX = np.finfo(np.float32).max
TAIL_CAP = 120                                # buffers; a tail that has not died by then fails its case


def subnormal(a):
    a = np.asarray(a)
    return (a != 0) & (np.abs(a) < TINY)


# ---- 1. numpy does not flush ---------------------------------------------------------------------------------------
def test_numpy_keeps_subnormals_in_this_process():
    v = np.full(8, 2.0 ** -126, np.float32) * np.full(8, 0.5, np.float32)          # an array: the vector units too
    assert np.array_equal(bits(v), np.full(8, 0x00400000, np.uint32))
    assert bits(f32(2.0 ** -126) * f32(0.5))[()] == 0x00400000
    assert bits(np.full(8, 2.0 ** -149, np.float32) + np.full(8, 2.0 ** -149, np.float32))[0] == 2
    assert bits(np.full(8, -2.0 ** -149, np.float32) * np.full(8, 0.25, np.float32))[0] == 0x80000000


# ---- 2. every fma32 against exact arithmetic -------------------------------------------------------------------------
FMAS = {"test_mix_host.fma32": test_mix_host.fma32, "test_meter_host.fma32": test_meter_host.fma32,
        "test_resample_host.fma32": test_resample_host.fma32, "test_reverb_host.fma": test_reverb_host.fma}


def fma_exact(a, b, c):
    """fmaf(a, b, c) of three float32 by IEEE 754's rules, the finite cases in rational arithmetic."""
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return f32(np.float64(a) * np.float64(b) + np.float64(c))             # no rounding enters: inf or NaN
    q = Fraction(a) * Fraction(b) + Fraction(c)
    if q == 0:
        # an exact zero is +0 unless both addends are -0: the product is a zero with the product of the signs
        product_is_neg_zero = (a == 0 or b == 0) and (np.signbit(a) != np.signbit(b))
        return f32(-0.0) if product_is_neg_zero and c == 0 and np.signbit(c) else f32(0.0)
    with np.errstate(over="ignore"):
        return round32_exact(q)


def pow2(rng, lo, hi, n):
    """n float32 of both signs with exponents in [lo, hi) and random mantissas."""
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.randint(lo, hi, n))).astype(np.float32)


def sub(rng, n):
    """n float32 that are whole multiples of 2^-149 below 2^-127, of both signs."""
    return (rng.randint(-(1 << 22), 1 << 22, n) * 2.0 ** -149).astype(np.float32)


def fma_ranges():
    """{name: (a, b, c)}: a few thousand seeded cases per range, the named ones among them."""
    rng = np.random.RandomState(20)
    n = 3000
    out = {}
    c = sub(rng, n)
    c[::7] = 0.0
    out["the product underflows"] = (pow2(rng, -100, -64, n), pow2(rng, -100, -64, n), c)
    out["the result is subnormal"] = (rng.uniform(-2, 2, n).astype(np.float32), pow2(rng, -133, -128, n), sub(rng, n))
    odd = (2 * rng.randint(0, 1 << 11, n) + 1).astype(np.float32)
    out["ties at the subnormal spacing"] = (odd * (rng.choice([-1.0, 1.0], n) * 2.0 ** -75).astype(np.float32),
                                            np.full(n, 2.0 ** -75, np.float32), sub(rng, n))   # odd * 2^-150 + c
    a, b = pow2(rng, -82, -72, n), pow2(rng, -78, -74, n)
    a[:500] = np.float32(2.0 ** -75) * rng.choice([-1.0, 1.0], 500)                # 2^-150 exactly: the tie goes to zero
    b[:500] = np.float32(2.0 ** -75)
    out["underflow to a signed zero"] = (a, b, rng.choice([0.0, -0.0], n).astype(np.float32))
    a = rng.randint(-4095, 4096, n).astype(np.float32) * np.exp2(rng.randint(-40, 40, n)).astype(np.float32)
    b = rng.randint(-4095, 4096, n).astype(np.float32) * np.exp2(rng.randint(-40, 40, n)).astype(np.float32)
    c = -(a * b)                                                                    # exact: 24 bits
    a[:400] = rng.choice([0.0, -0.0], 400)
    c[:400] = rng.choice([0.0, -0.0], 400)
    b[200:600] = rng.choice([0.0, -0.0], 400)
    c[400:600] = rng.choice([0.0, -0.0], 200)
    out["exact cancellations"] = (a, b, c)
    a, b, c = pow2(rng, 63, 64, n), np.abs(pow2(rng, 63, 65, n)), pow2(rng, 100, 128, n)
    named = [(FLT_MAX, 1.0, 2.0 ** 102), (FLT_MAX, 1.0, 2.0 ** 103), (-FLT_MAX, 1.0, -2.0 ** 102),
             (-FLT_MAX, 1.0, -2.0 ** 103), (FLT_MAX, 1.0, FLT_MAX), (2.0 ** 64, 2.0 ** 63, 2.0 ** 127)]
    for k, v in enumerate(named):
        a[k], b[k], c[k] = v
    out["the two sides of the overflow boundary"] = (a, b, c)
    a = (rng.uniform(1.0, 1.2, n) * 2.0 ** 64).astype(np.float32)
    b = (rng.uniform(1.0, 1.2, n) * 2.0 ** 64 * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    c = (-np.sign(b) * rng.uniform(0.6, 1.0, n) * float(FLT_MAX)).astype(np.float32)
    a[0], b[0], c[0] = FLT_MAX, 2.0, -FLT_MAX
    a[1], b[1], c[1] = -FLT_MAX, 2.0, FLT_MAX
    out["a product that overflows alone"] = (a, b, c)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0, FLT_MAX, 2.0 ** -149], np.float32)
    idx = np.array([(i, j, k) for i in range(9) for j in range(9) for k in range(9)])
    idx = idx[(idx < 3).any(axis=1)]                                                # at least one operand not finite
    out["operands that are not finite"] = tuple(special[idx[:, k]] for k in range(3))
    return out


@functools.lru_cache(maxsize=None)
def fma_truth():
    return {name: (abc, np.array([fma_exact(*v) for v in zip(*abc)], np.float32)) for name, abc in fma_ranges().items()}


def test_the_fma_ranges_are_what_they_are_named_for():
    t = {name: want for name, (_, want) in fma_truth().items()}
    (a, b, _), z = fma_truth()["the product underflows"]
    assert (np.abs(a.astype(np.float64) * b.astype(np.float64)) < 2.0 ** -126).all() and subnormal(z).mean() > 0.3
    assert subnormal(t["the result is subnormal"]).mean() > 0.8
    (a, b, c), _ = fma_truth()["ties at the subnormal spacing"]
    assert all((Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) / Fraction(2) ** -149 % 1 == Fraction(1, 2)
               for x, y, z in list(zip(a, b, c))[:200])
    z = t["underflow to a signed zero"]
    assert ((z == 0) & np.signbit(z)).sum() > 200 and ((z == 0) & ~np.signbit(z)).sum() > 200 and (z != 0).sum() > 200
    z = t["exact cancellations"]
    assert not z.any() and 10 < np.signbit(z).sum() < 400
    z = t["the two sides of the overflow boundary"]
    assert np.array_equal(z[:6], np.array([FLT_MAX, np.inf, -FLT_MAX, -np.inf, np.inf, np.inf], np.float32))
    assert np.isinf(z).sum() > 100 and np.isfinite(z).sum() > 100
    (a, b, c), z = fma_truth()["a product that overflows alone"]
    with np.errstate(over="ignore"):
        assert np.isinf(a * b).all() and np.isfinite(z).all() and z[0] == FLT_MAX and z[1] == -FLT_MAX
    z = t["operands that are not finite"]
    assert (~np.isfinite(z)).all() and np.isnan(z).sum() > 100 and np.isinf(z).sum() > 50


@pytest.mark.parametrize("name", sorted(FMAS))
def test_every_fma32_is_exact_at_the_edges(name):
    fma = FMAS[name]
    for rng_name, ((a, b, c), want) in fma_truth().items():
        with np.errstate(invalid="ignore", over="ignore"):
            got = fma(a, b, c)
        assert got.dtype == np.float32
        bad = np.flatnonzero(~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))
        assert not bad.size, (name, rng_name, [(a[k], b[k], c[k], got[k], want[k]) for k in bad[:5]])


def test_what_the_issue_names():
    fma = test_mix_host.fma32
    assert fma(FLT_MAX, 1.0, 2.0 ** 102) == FLT_MAX and fma(FLT_MAX, 1.0, 2.0 ** 103) == np.inf
    assert fma(FLT_MAX, 2.0, -FLT_MAX) == FLT_MAX
    assert fma(np.inf, 1.0, 0.0) == np.inf and fma(1.0, 1.0, np.inf) == np.inf and fma(-np.inf, 1.0, 0.0) == -np.inf
    assert np.isnan(fma(np.inf, 1.0, -np.inf)) and np.isnan(fma(np.inf, 0.0, 1.0))
    assert bits(fma(0.0, 0.5, -0.0))[()] == 0 and bits(fma(-0.0, 0.5, -0.0))[()] == 0x80000000


# ---- 3. the cases ----------------------------------------------------------------------------------------------------
def mix_form(buses):
    """k_mix.hip, mix_pick_form; the device tests hold plan.form to this."""
    return (64, 4) if buses > 32 else (32, 8)


class Tape:
    """Records the calls made on an actor (and what its run() returned): the script a device actor replays."""

    def __init__(self, actor):
        self.actor, self.ops, self.outs = actor, [], []

    def __getattr__(self, name):
        def call(*args):
            self.ops.append((name,) + args)
            r = getattr(self.actor, name)(*args)
            if name == "run":
                self.outs.append(r)
        return call

    def dead(self):
        return self.actor.dead()


def quiet(*arrays):
    """Every value subnormal or zero."""
    return all(bool((np.abs(a) < TINY).all()) for a in arrays)


def mix_first_refused(g):
    """The host twins of the device rules that had none yet (k_mix.hip, k_delay.hip, k_dynamics.hip; the contract's
    column `admitted` in include/gab_c_api.h): the index into the flat table of the first refused value, or None."""
    hits = np.flatnonzero(~np.isfinite(np.asarray(g, np.float32).ravel()))
    return int(hits[0]) if hits.size else None


def delay_first_refused(p, interp, max_delay):
    t = np.asarray(p, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(t)
        bad[:, 0] |= ~((t[:, 0] >= f32(2 if interp == "lagrange3" else 1)) & (t[:, 0] <= f32(max_delay)))
        bad[:, 1] |= ~(np.abs(t[:, 1]) < f32(1.0))
    hits = np.flatnonzero(bad.ravel())
    return int(hits[0]) if hits.size else None


def dyn_first_refused(p):
    t = np.asarray(p, np.float32).reshape(-1, 8)
    cap = f32(1.0 - 2.0 ** -20)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(t)
        bad[:, 0] |= ~(np.abs(t[:, 0]) <= f32(128.0))
        bad[:, 1] |= ~((t[:, 1] >= f32(-1.0)) & (t[:, 1] <= 0))
        bad[:, 2] |= ~((t[:, 2] >= 0) & (t[:, 2] <= f32(64.0)))
        bad[:, 3] |= ~(t[:, 3] >= 0)
        bad[:, 4] |= ~((t[:, 4] >= 0) & (t[:, 4] <= cap))
        bad[:, 5] |= ~((t[:, 5] >= 0) & (t[:, 5] <= cap))
        bad[:, 7] |= ~(t[:, 7] <= 0)
    hits = np.flatnonzero(bad.ravel())
    return int(hits[0]) if hits.size else None


class Host:
    """What the host actors share: the two markers of a tape, a batch as its buffers one by one, and a refused set, which
    the plan's host rule must refuse and which changes nothing."""

    def cut(self):
        pass

    def check(self, want=None):
        self.__dict__.setdefault("checks", []).append(self.state())

    def run_batch(self, xs, keys):
        return [self.run(x, k) for x, k in zip(xs, keys)]

    def refused(self, p, first_track, ramp):
        assert self.rule(p) is not None

    def params_tracks(self, p, first_track, ramp):
        self.twin.set_params(p, ramp=ramp, first_track=first_track)


class HostMix(Host):
    def __init__(self, T, B, M, layout="track"):
        self.twin = MixTwin(T, B, M, *mix_form(M))

    def gains(self, g, ramp):
        self.twin.set_gains(g, ramp=ramp)

    def gains_tracks(self, g, first_track, ramp):
        self.twin.set_gains(g, ramp=ramp, first=first_track)

    def rule(self, g):
        return mix_first_refused(g)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        with np.errstate(invalid="ignore", over="ignore"):
            return {"y": self.twin.process(x)}

    def state(self):
        return {"current": self.twin.cur.copy(), "target": self.twin.tgt.copy()}

    def dead(self):
        return True


class HostDelay(Host):
    def __init__(self, T, B, M, interp):
        self.twin = DelayTwin(T, B, M, interp)

    def params(self, p, ramp):
        self.twin.set_params(p, ramp=ramp)

    def rule(self, p):
        return delay_first_refused(p, self.twin.interp, self.twin.M)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        with np.errstate(invalid="ignore", over="ignore"):
            return {"y": self.twin.process(x)}

    def state(self):
        t = self.twin
        return {"current": t.cur.copy(), "target": t.tgt.copy(), "line": t.line.hist.copy(),
                "pos": np.full(t.T, t.line.count % delay_capacity(t.B, t.M), np.int64)}

    def dead(self):
        return quiet(self.twin.line.hist)


class FlushedDelay(HostDelay):
    """The negative control: a delay line that flushes its subnormals to zero after every buffer."""

    def run(self, x, key=None):
        out = HostDelay.run(self, x)
        h = self.twin.line.hist
        self.twin.line.hist = np.where(np.abs(h) < TINY, f32(0.0), h).astype(np.float32)
        return out


class HostMeter(Host):
    def __init__(self, T, B, W):
        self.twin = MeterTwin(T, B, W)

    def decay(self, v):
        self.twin.set_decay(v)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        with np.errstate(invalid="ignore", over="ignore"):
            return {"rows": self.twin.process(x)}

    def state(self):
        t = self.twin
        return {"hist": t.hist.copy(), "hold": t.hold.copy(), "true_peak_max": t.tpmax.copy(), "filter": t.filter.copy(),
                "ring": t.ring.copy(), "pos": np.full(t.T, t.pos, np.int64)}

    def dead(self):
        t = self.twin                                             # true_peak_max is a running maximum: it never decays
        return quiet(t.hist, t.hold, t.filter, t.ring)


class HostResample(Host):
    def __init__(self, T, B, up, down, K):
        self.twin = ResampleTwin(T, B, up, down, K=K)

    def taps(self, t):
        self.twin.set_taps(t)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        with np.errstate(invalid="ignore", over="ignore"):
            rows, n = self.twin.process(x)
        return {"y": rows, "count": np.array([n], np.int64)}

    def state(self):
        return {"hist": self.twin.hist.copy(), "k": np.array([self.twin.k], np.int64)}

    def dead(self):
        return True


class HostDyn(Host):
    def __init__(self, T, B, link, keyed):
        self.twin = DynTwin(T, B, link)

    def params(self, p, ramp):
        self.twin.set_params(p, ramp=ramp)

    def rule(self, p):
        return dyn_first_refused(p)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        y, gr = self.twin.process(x, key)
        return {"y": y, "gr": gr}

    def state(self):
        t = self.twin
        return {"current": t.cur.copy(), "target": t.tgt.copy(), "s": t.s.copy()}

    def dead(self):
        return quiet(self.twin.s)


class HostReverb(Host):
    def __init__(self, T, B, N, O, M):
        self.twin = ReverbTwin(T, B, N, O, M)

    def params(self, p, ramp):
        self.twin.set_params(p, ramp=ramp)

    def delays(self, d):
        self.twin.set_delays(d)

    def delays_tracks(self, d, first_track):
        self.twin.set_delays(d, first_track=first_track)

    def rule(self, p):
        return reverb_first_refused(p, self.twin.N, self.twin.O)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        return {"y": self.twin.process(x)}

    def state(self):
        t = self.twin
        return {"current": t.cur.copy(), "target": t.tgt.copy(), "lines": t.hist.copy(), "q": t.q.copy(),
                "pos": np.full(t.T, t.pos, np.int64), "delays": t.delays.copy()}

    def dead(self):
        return quiet(self.twin.hist, self.twin.q)


class HostGate(Host):
    def __init__(self, T, B, link, keyed):
        self.twin = GateTwin(T, B, link)

    def params(self, p, ramp):
        self.twin.set_params(p, ramp=ramp)

    def rule(self, p):
        return gate_first_refused(p)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        with np.errstate(invalid="ignore", over="ignore"):
            y, act = self.twin.process(x, key)
        return {"y": y, "act": act}

    def state(self):
        t = self.twin
        return {"current": t.cur.copy(), "target": t.tgt.copy(), "gain": t.g.copy(), "count": t.c.copy()}

    def dead(self):
        return True


class HostLim(Host):
    def __init__(self, T, B, W, link):
        self.twin = limiter_twin.Twin(T, B, W, link)

    def params(self, p, ramp):
        self.twin.set_params(p, ramp=ramp)

    def rule(self, p):
        return limiter_twin.first_refused(p)

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        y, gr = self.twin.process(x)
        return {"y": y, "gr": gr}

    def state(self):
        t = self.twin
        xd, th, e = t.hist
        return {"current": t.cur.copy(), "target": t.tgt.copy(), "xd": xd.copy(), "t": th.copy(), "e": e.copy()}

    def dead(self):
        return True


XOVER_NO_ROW = np.array([1.0, 0.0, 0.0], np.float32)          # what a first ranged set leaves on the rows it did not name


class HostXover(Host):
    """The crossover's life-cycle on the host: no rows until a set is accepted (unset_run() is a run on such a plan:
    refused, nothing changes), a refused set is no set, a set keeps the state."""

    def __init__(self, T, B, K):
        self.twin = XoverTwin(T, B, K)

    def splits(self, rows):
        self.twin.set_splits(rows)

    def splits_tracks(self, rows, first_track):
        self.twin.set_splits(rows, first_track=first_track)

    def refused(self, rows, first_track):
        assert xover_first_refused(rows) is not None

    def unset_run(self, x):
        assert self.twin.rows is None

    def reset(self):
        self.twin.reset()

    def run(self, x, key=None):
        return {"bands": self.twin.process(x)}

    def state(self):
        t = self.twin
        rows = np.tile(XOVER_NO_ROW, (t.T, t.S, 1)) if t.rows is None else t.rows.copy()
        return {"state": t.state.copy(), "rows": rows, "has_rows": np.array([t.rows is not None], np.int64)}

    def dead(self):
        return quiet(self.twin.state)


class HostSpec(Host):
    """The spectrum plan's carried state (spectrum_twin.Framer) with the window and the edges in force.  run() returns
    the call's frame count and its frames' 1024 raw samples each (history plus call), which a device actor feeds to a
    single-frame plan: the transform is no bit twin, the framing is."""

    def __init__(self, T, B, H, mode, bands):
        self.framer, self.mode, self.bands = spectrum_twin.Framer(T, B, H), mode, bands
        self.band_edges = spectrum_twin.default_edges(bands) if bands else None

    def window(self, w):
        assert spectrum_twin.bad_window(w) is None
        self.framer.w = np.array(w, np.float32)

    def edges(self, e):
        assert spectrum_twin.bad_edge(list(e), self.bands) == -1
        self.band_edges = [int(v) for v in e]

    def refused_window(self, w):
        assert spectrum_twin.bad_window(w) is not None

    def refused_edges(self, e):
        assert spectrum_twin.bad_edge(list(e), self.bands) >= 0

    def reset(self):
        self.framer.reset()

    def run(self, x, key=None):
        f = self.framer
        both = np.concatenate([f.hist, np.asarray(x, np.float32)], axis=1)
        ends = spectrum_twin.frame_ends(f.p, f.B, f.H)
        at = [e - f.p + spectrum_twin.HIST for e in ends]
        raw = np.zeros((len(at), f.T, spectrum_twin.N), np.float32)
        for j, c in enumerate(at):
            raw[j] = both[:, c - spectrum_twin.N:c]
        assert len(ends) == spectrum_twin.count(f.p, f.B, f.H)
        taken = f.take(x[None])
        assert same(taken, f.w[None, None, :] * raw)              # the Framer's own frames are these under its window
        return {"count": np.array([len(ends)], np.int64), "raw": raw}

    def state(self):
        f = self.framer
        return {"hist": f.hist.copy(), "window": f.w.copy(), "pos": np.array([f.p % f.H], np.int64)}

    def dead(self):
        return True


HOSTS = {"mix": HostMix, "delay": HostDelay, "meter": HostMeter, "resample": HostResample, "dyn": HostDyn,
         "reverb": HostReverb, "gate": HostGate, "lim": HostLim, "xover": HostXover, "spec": HostSpec}


def lvl(rng, shape, e):
    """Uniform noise in (-2^e, 2^e)."""
    return (rng.uniform(-1.0, 1.0, shape) * 2.0 ** e).astype(np.float32)


def zero_blocks(T, B, rng):
    """+0.0 everywhere, -0.0 everywhere, and zeros of random signs."""
    pz = np.zeros((T, B), np.float32)
    nz = -pz
    rz = np.where(rng.randint(0, 2, (T, B)) == 1, f32(-0.0), f32(0.0)).astype(np.float32)
    return pz, nz, rz


def sprinkle(p, rng, cols=None, every=4):
    """One value in `every` of the admitted columns becomes -0.0."""
    p = np.array(p, np.float32)
    cols = np.arange(p.shape[1]) if cols is None else np.asarray(cols)
    hit = rng.randint(0, every, (p.shape[0], len(cols))) == 0
    sub_p = p[:, cols]
    sub_p[hit] = -0.0
    p[:, cols] = sub_p
    return p


def some_rows(old, new, rng):
    """Half of the rows move to `new`; the others stay, their -0.0 included."""
    move = rng.randint(0, 2, old.shape[0]).astype(bool)
    return np.where(move[:, None], new, old).astype(np.float32)


def zeros_script(t, T, B, rng, setter, p0, p1, p2):
    """The zeros regime of a ramped plan: steady, ramp, behind the ramp, ramp again, behind it."""
    pz, nz, ck = zero_blocks(T, B, rng)
    setter(p0, False)
    t.run(pz, None)
    t.run(nz, None)
    setter(p1, True)
    t.run(pz, None)
    t.run(nz, None)
    setter(p2, True)
    t.run(nz, None)
    t.run(ck, None)


def die(t, T, B, key=None):
    """Silence until the carried state is subnormal or zero everywhere, and two buffers more."""
    z = np.zeros((T, B), np.float32)
    n = 0
    while not t.dead():
        n += 1
        assert n <= TAIL_CAP, "the tail does not die"
        t.run(z, key)
    t.run(z, key)
    t.run(z, key)


def dirty_block(x, dirty):
    x = x.copy()
    if dirty:
        x[64, 17], x[-1, 40] = np.nan, np.inf
    return x


def build_mix(t, regime, rng, dirty, T, B, M, layout="track"):
    g = [sprinkle(gains(T, M, rng.randint(1 << 30)), rng) for _ in range(3)]
    if regime == "tail":
        t.gains(g[0], False)
        t.run(lvl(rng, (T, B), -122), None)                       # products with the gains are subnormal
        t.gains(lvl(rng, (T, M), -125), False)                    # and gains that are themselves subnormal
        t.run(lvl(rng, (T, B), 0), None)
        t.gains(lvl(rng, (T, M), -125), True)                     # a ramp whose target - current is subnormal
        t.run(lvl(rng, (T, B), 0), None)
        t.run(lvl(rng, (T, B), 0), None)
    elif regime == "flt_max":
        t.gains(g[0], False)
        t.run(lvl(rng, (T, B), 126), None)
        t.gains(g[1], True)
        t.run(lvl(rng, (T, B), 126), None)
        t.run(lvl(rng, (T, B), 125), None)
    elif regime == "zeros":
        zeros_script(t, T, B, rng, t.gains, g[0], some_rows(g[0], g[1], rng), some_rows(g[1], g[2], rng))
    else:                                                         # contain / contain_ramp
        g[0][64, 0] = 0.0                                         # the NaN's track has no gain on bus 0
        t.gains(g[0], False)
        t.run(lvl(rng, (T, B), 0), None)
        if regime == "contain_ramp":
            t.gains(g[1], True)
        t.run(dirty_block(lvl(rng, (T, B), 0), dirty), None)
        t.run(lvl(rng, (T, B), 0), None)


def build_delay(t, regime, rng, dirty, T, B, M, interp):
    p = [delay_mix(T, B, M, interp, rng.randint(1 << 20)) for _ in range(3)]
    if regime == "tail":
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), -100), None)
        die(t, T, B)
    elif regime == "flt_max":
        p[0][:, 2:] *= f32(2.0)                                   # wet and dry up to 2: the output crosses FLT_MAX
        t.params(p[0], False)
        for _ in range(3):
            t.run(lvl(rng, (T, B), 127), None)
        t.run(lvl(rng, (T, B), 0), None)                          # with feedback the damage stays; without, it leaves
        t.run(lvl(rng, (T, B), 0), None)
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    elif regime == "zeros":
        p = [sprinkle(q, rng, cols=(1, 2, 3)) for q in p]
        zeros_script(t, T, B, rng, t.params, p[0], some_rows(p[0], p[1], rng), some_rows(p[1], p[2], rng))
    else:
        p[0][64, 1], p[0][-1, 1] = 0.0, 0.5                      # the NaN's track without feedback, the infinity's with
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), 0), None)
        t.run(dirty_block(lvl(rng, (T, B), 0), dirty), None)
        for _ in range(3):
            t.run(lvl(rng, (T, B), 0), None)
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)


def build_meter(t, regime, rng, dirty, T, B, W):
    if regime == "tail":
        t.decay(0.5)
        t.run(lvl(rng, (T, B), 0) * np.exp2(rng.uniform(-80.0, -62.0, (T, 1))).astype(np.float32), None)
        die(t, T, B)
    elif regime == "flt_max":
        t.decay(0.5)
        t.run(lvl(rng, (T, B), 127), None)                        # finite: squares and the filter overflow inside
        t.run(lvl(rng, (T, B), 127), None)
        x = lvl(rng, (T, B), 0)
        x[64, 10], x[-1, 70] = np.inf, np.nan                     # and samples that are not finite themselves
        t.run(x, None)
        t.run(lvl(rng, (T, B), 0), None)                          # the filter stays poisoned
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    else:
        pz, nz, ck = zero_blocks(T, B, rng)
        t.decay(0.5)
        for x in (pz, nz, ck, lvl(rng, (T, B), -140), nz):
            t.run(x, None)


def build_resample(t, regime, rng, dirty, T, B, up, down, K):
    if regime == "tail":
        for e in (-125, -128, -125):
            t.run(lvl(rng, (T, B), e), None)
    elif regime == "flt_max":
        for _ in range(3):
            t.run(lvl(rng, (T, B), 128) * f32(0.99), None)
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    else:
        pz, nz, ck = zero_blocks(T, B, rng)
        for x in (pz, nz, ck, nz):
            t.run(x, None)


def build_dyn(t, regime, rng, dirty, T, B, link, keyed):
    p = [dyn_mix(T, rng.randint(1 << 20)) for _ in range(3)]

    def key(e):
        return lvl(rng, (T, B), e) if keyed else None
    if regime == "tail":
        for q in p:
            q[:, 5] = rng.choice([0.25, 0.5, 0.75], T)            # a fast release
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), 0), key(0))                        # full scale, over every threshold
        die(t, T, B, np.zeros((T, B), np.float32) if keyed else None)
    elif regime == "quiet":
        p[0][:, 0] = rng.uniform(-110.0, -98.0, T)                # thresholds below the detector's floor of -96
        p[0][:, 7] = -256.0
        t.params(p[0], False)
        for _ in range(3):
            t.run(lvl(rng, (T, B), -120), key(-120))
    elif regime == "flt_max":
        for q in p:
            q[:, 6] = rng.uniform(1.0, 8.0, T) * rng.choice([-1.0, 1.0], T)
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), 126), key(-3))
        t.params(p[1], True)
        t.run(lvl(rng, (T, B), 126), key(-3))
        t.run(lvl(rng, (T, B), 0), key(0))                        # nothing carried was reached: finite at once
        t.reset()
        t.run(lvl(rng, (T, B), 0), key(0))
    else:
        for q in p:
            q[:, 0] = rng.uniform(-110.0, -90.0, T)               # silence reads -96: over some thresholds
            q[:, 6] *= rng.choice([-1.0, 1.0], T)
        p = [sprinkle(q, rng) for q in p]
        zeros_script(t, T, B, rng, t.params, p[0], some_rows(p[0], p[1], rng), some_rows(p[1], p[2], rng))
        if keyed:                                                 # and once with a key that is not silence
            t.run(zero_blocks(T, B, rng)[2], lvl(rng, (T, B), 0))


def build_reverb(t, regime, rng, dirty, T, B, N, O, M):
    loop = 0.5 if regime == "tail" else 0.9
    p = [reverb_mix(T, N, O, rng.randint(1 << 20), loop=loop) for _ in range(3)]
    t.delays(rng.randint(REVERB_MIN_DELAY, M + 1, (T, N)).astype(np.int32))
    if regime == "tail":
        p[0][:, N:2 * N] = rng.uniform(0.1, 0.6, (T, N))          # damping on
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), -100), None)
        die(t, T, B)
    elif regime == "flt_max":
        p[0][:, 2 * N:3 * N] *= f32(3.0)                          # input gains up to 3: the lines cross FLT_MAX
        p[0][:, 3 * N:] *= f32(6.0)                               # and output gains with which the outputs do
        t.params(p[0], False)
        for _ in range(3):
            t.run(lvl(rng, (T, B), 126), None)
        t.run(lvl(rng, (T, B), 0), None)                          # the damage comes round for ever
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    else:
        p = [sprinkle(q, rng) for q in p]
        for q in p:                                               # two tracks on which every term of an output is -0:
            q[:2, :N] = -np.abs(q[:2, :N]) - f32(0.01)            # g < 0, so v = g (+0) = -0; damp = -0.0, so
            q[:2, N:2 * N] = -0.0                                 # q = fmaf(-0.0, +0, -0) = -0; b, c, dry > 0
            q[:2, 2 * N:] = np.abs(q[:2, 2 * N:]) + f32(0.01)
        zeros_script(t, T, B, rng, t.params, p[0], some_rows(p[0], p[1], rng), some_rows(p[1], p[2], rng))


def build_lim(t, regime, rng, dirty, T, B, W, link):
    p = [limiter_twin.lim_mix(T, rng.randint(1 << 20)) for _ in range(3)]
    if regime == "flt_max":
        ends = np.where(np.arange(T) % 2 == 0, 2.0 ** -32, 2.0 ** 32).astype(np.float32)
        for k, q in enumerate(p):
            q[:, limiter_twin.DRIVE] = rng.uniform(1.0, 4.0, T)       # drive above 1: xd = drive x crosses FLT_MAX
            q[:, limiter_twin.CEIL] = ends if k % 2 == 0 else ends[::-1]   # both ends of the admitted range, swapped
        t.params(p[0], False)
        t.run(lvl(rng, (T, B), 126), None)
        t.params(p[1], True)                                      # every ceiling ramps from one end to the other
        t.run(lvl(rng, (T, B), 127), None)
        t.run(lvl(rng, (T, B), 126), None)
        for _ in range(2):                                        # the infinities sit in the xd history for W - 1 samples
            t.run(lvl(rng, (T, B), 0), None)
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    else:
        p = [sprinkle(q, rng, cols=(limiter_twin.DRIVE, limiter_twin.REL)) for q in p]      # (no ceiling is -0.0)
        zeros_script(t, T, B, rng, t.params, p[0], some_rows(p[0], p[1], rng), some_rows(p[1], p[2], rng))


def xover_edge_rows(T, K, rng):
    """[T][K - 1][3]: the splits of test_crossover_host.SETS that lie against both ends of the band (20 Hz and 23 kHz)
    on the even tracks, splits drawn per track on the odd ones."""
    S = K - 1
    f = np.sort(np.exp(rng.uniform(np.log(30.0), np.log(18000.0), (T, S))), axis=1)
    f[::2] = {1: [20.0], 2: [20.0, 23000.0], 3: [20.0, 25.0, 23000.0]}[S]
    if S == 1:
        f[::4] = 23000.0
    return np.stack([xover_rows32(row) for row in f])


def build_xover(t, regime, rng, dirty, T, B, K):
    rows = [xover_edge_rows(T, K, rng) for _ in range(2)]
    if regime == "flt_max":
        t.splits(rows[0])
        t.run(lvl(rng, (T, B), 126), None)
        t.run(lvl(rng, (T, B), 127), None)                        # finite: the integrators overflow inside
        t.splits(rows[1])                                         # a set keeps the state, the infinities in it too
        t.run(lvl(rng, (T, B), 126), None)
        for _ in range(2):
            t.run(lvl(rng, (T, B), 0), None)                      # a NaN in an integrator stays for good
        t.reset()
        t.run(lvl(rng, (T, B), 0), None)
    else:
        pz, nz, ck = zero_blocks(T, B, rng)
        t.splits(rows[0])
        for x in (pz, nz, ck):
            t.run(x, None)
        t.splits(rows[1])
        for x in (nz, ck, pz):                                    # the buffers behind a set
            t.run(x, None)


BUILDERS = {"mix": build_mix, "delay": build_delay, "meter": build_meter, "resample": build_resample, "dyn": build_dyn,
            "reverb": build_reverb, "lim": build_lim, "xover": build_xover}

Case = collections.namedtuple("Case", "plan regime shape seed offset want")
COUNTS = ("subnormal outputs", "subnormal state words", "+inf", "-inf", "NaN", "-0.0")


def case_id(c):
    return "-".join([c.plan, c.regime] + [str(v) for v in c.shape]) + ("-offset" if c.offset else "")


@functools.lru_cache(maxsize=None)
def _reference(plan, regime, shape, seed, dirty):
    host = HOSTS[plan](*shape)
    tape = Tape(host)
    BUILDERS[plan](tape, regime, np.random.RandomState(seed), dirty, *shape)
    for op in tape.ops:
        for a in op[1:]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return tape.ops, tape.outs, host.state(), host


def reference(case, dirty=True):
    """(the tape of calls, run()'s outputs per buffer, the carried state at the end, the host actor); read only."""
    return _reference(case.plan, case.regime, case.shape, case.seed, dirty)


def play(ops, actor, batch=False):
    """The tape on another actor; batch: consecutive run() calls go to run_batch(xs, keys) as one.  Returns the outputs.
    Two markers (tests/walks.py): ("cut",) ends the current batch and is not passed on; ("check", state) is passed on
    behind the batch, as every call that is not a run() is: a device actor compares its carried state there."""
    outs, pending = [], []

    def flush():
        if pending:
            outs.extend(actor.run_batch([p[0] for p in pending], [p[1] for p in pending]))
            del pending[:]
    for op in ops:
        if op[0] == "run" and batch:
            if pending and (pending[-1][1] is None) != (op[2] is None):        # a batch has a key for every buffer or none
                flush()
            pending.append(op[1:])
            continue
        flush()
        if op[0] == "cut":
            continue
        r = getattr(actor, op[0])(*op[1:])
        if op[0] == "run":
            outs.append(r)
    flush()
    return outs


def differing(got, want):
    """The (buffer, name) pairs at which two lists of outputs differ under same()."""
    assert len(got) == len(want)
    return [(k, name) for k, (g, w) in enumerate(zip(got, want)) for name in sorted(w) if not same(g[name], w[name])]


def counts(outs, state):
    fl = [a for o in outs for a in o.values() if a.dtype == np.float32]
    st = [a for a in state.values() if a.dtype == np.float32]
    return (int(sum(subnormal(a).sum() for a in fl)), int(sum(subnormal(a).sum() for a in st)),
            int(sum((a == np.inf).sum() for a in fl)), int(sum((a == -np.inf).sum() for a in fl)),
            int(sum(np.isnan(a).sum() for a in fl)), int(sum(((a == 0) & np.signbit(a)).sum() for a in fl)))


# plan, regime, shape, seed, a pointer 4 bytes off, the pinned counts (COUNTS' order).
# Shapes.  mix: (tracks, bufsize, buses, layout); delay: (tracks, bufsize, max_delay, interp); meter: (tracks, bufsize,
# window); resample: (tracks, bufsize, up, down, taps); dyn: (tracks, bufsize, link, keyed); reverb: (tracks, bufsize,
# lines, outs, max_delay); lim: (tracks, bufsize, W, link); xover: (tracks, bufsize, bands).  130 tracks: two full owners
# of 64 and a partial one; reverb gives a wave 64 / lines tracks: 34 tracks of 4 lines, 9 of 16; a limiter's wave owns
# 8 tracks, and 128 tracks at link 64 take its detector launch in front; a crossover's wave owns 64, 32 or 16 tracks
# for 2, 3 or 4 bands.  bufsize 100: scalar loads and a partial last chunk; 128: the vector forms.
CASES = [
    Case("mix", "tail", (130, 100, 2, "track"), 1, False, (68, 254, 0, 0, 0, 0)),
    Case("mix", "tail", (130, 128, 33, "sample"), 2, True, (1496, 4242, 0, 0, 0, 0)),
    Case("mix", "flt_max", (130, 100, 33, "track"), 3, False, (0, 0, 924, 908, 38, 0)),
    Case("mix", "flt_max", (130, 128, 2, "sample"), 4, False, (0, 0, 66, 71, 1, 0)),
    Case("mix", "zeros", (130, 100, 2, "sample"), 5, False, (0, 0, 0, 0, 0, 0)),
    Case("mix", "zeros", (130, 128, 33, "track"), 6, False, (0, 0, 0, 0, 0, 0)),
    Case("mix", "contain", (130, 100, 2, "track"), 7, False, (0, 0, 0, 2, 2, 0)),
    Case("mix", "contain", (130, 100, 33, "sample"), 8, False, (0, 0, 9, 18, 39, 0)),
    Case("mix", "contain_ramp", (130, 128, 2, "sample"), 9, False, (0, 0, 1, 1, 2, 0)),
    Case("mix", "contain_ramp", (130, 128, 33, "track"), 10, False, (0, 0, 12, 20, 34, 0)),
    Case("delay", "tail", (130, 100, 64, "linear"), 11, False, (129890, 4180, 0, 0, 0, 70132)),
    Case("delay", "tail", (130, 100, 64, "lagrange3"), 12, True, (110357, 3611, 0, 0, 0, 77907)),
    Case("delay", "tail", (130, 128, 64, "linear"), 13, False, (113656, 3521, 0, 0, 0, 47010)),
    Case("delay", "tail", (130, 128, 64, "lagrange3"), 14, False, (145482, 3660, 0, 0, 0, 59959)),
    Case("delay", "flt_max", (130, 100, 64, "linear"), 15, False, (0, 0, 874, 843, 16891, 0)),
    Case("delay", "flt_max", (130, 128, 64, "lagrange3"), 16, False, (0, 0, 939, 975, 3169, 0)),
    Case("delay", "zeros", (130, 100, 64, "lagrange3"), 17, False, (0, 0, 0, 0, 0, 20075)),
    Case("delay", "zeros", (130, 128, 64, "linear"), 18, False, (0, 0, 0, 0, 0, 27025)),
    Case("delay", "contain", (130, 128, 64, "linear"), 19, False, (0, 0, 1, 0, 135, 0)),
    Case("delay", "contain", (130, 100, 64, "lagrange3"), 20, False, (0, 0, 1, 1, 105, 0)),
    Case("meter", "tail", (130, 100, 3), 21, False, (3989, 520, 0, 0, 0, 0)),
    Case("meter", "tail", (130, 128, 3), 22, True, (2903, 639, 0, 0, 0, 0)),
    Case("meter", "flt_max", (130, 100, 3), 23, False, (0, 0, 267, 0, 1041, 0)),
    Case("meter", "flt_max", (130, 128, 3), 24, False, (0, 0, 267, 0, 1041, 0)),
    Case("meter", "zeros", (130, 100, 3), 25, False, (910, 778, 0, 0, 0, 0)),
    Case("meter", "zeros", (130, 128, 3), 26, False, (910, 780, 0, 0, 0, 0)),
    Case("resample", "tail", (130, 100, 160, 147, 4), 27, False, (31564, 200, 0, 0, 0, 0)),
    Case("resample", "tail", (130, 128, 147, 160, 4), 28, True, (34585, 183, 0, 0, 0, 0)),
    Case("resample", "flt_max", (130, 100, 147, 160, 8), 29, False, (0, 0, 156, 156, 0, 0)),
    Case("resample", "flt_max", (130, 128, 160, 147, 8), 30, False, (0, 0, 399, 415, 0, 0)),
    Case("resample", "zeros", (130, 100, 160, 147, 4), 31, False, (0, 0, 0, 0, 0, 859)),
    Case("resample", "zeros", (130, 128, 147, 160, 4), 32, False, (0, 0, 0, 0, 0, 899)),
    Case("dyn", "tail", (130, 100, 1, False), 33, False, (88, 36, 0, 0, 0, 0)),
    Case("dyn", "tail", (130, 128, 2, True), 34, False, (113, 38, 0, 0, 0, 0)),
    Case("dyn", "quiet", (130, 128, 1, True), 35, True, (20918, 0, 0, 0, 0, 0)),
    Case("dyn", "quiet", (130, 100, 2, False), 36, False, (18381, 0, 0, 0, 0, 0)),
    Case("dyn", "flt_max", (130, 100, 2, False), 37, False, (0, 0, 464, 479, 0, 0)),
    Case("dyn", "flt_max", (130, 128, 1, True), 38, False, (0, 0, 1888, 1905, 0, 0)),
    Case("dyn", "zeros", (130, 100, 1, True), 39, False, (6, 2, 0, 0, 0, 43718)),
    Case("dyn", "zeros", (130, 128, 2, False), 40, False, (2, 4, 0, 0, 0, 47618)),
    Case("reverb", "tail", (34, 100, 4, 2, 64), 41, False, (49590, 7460, 0, 0, 0, 503)),
    Case("reverb", "tail", (9, 128, 16, 1, 64), 42, True, (5996, 9330, 0, 0, 0, 10)),
    Case("reverb", "flt_max", (9, 100, 16, 2, 64), 43, False, (0, 0, 47, 83, 1650, 0)),
    Case("reverb", "flt_max", (34, 128, 4, 1, 64), 44, False, (0, 0, 398, 420, 1601, 0)),
    Case("reverb", "zeros", (34, 128, 4, 2, 64), 45, False, (0, 0, 0, 0, 0, 3457)),
    Case("reverb", "zeros", (9, 100, 16, 1, 64), 46, False, (0, 0, 0, 0, 0, 308)),
    Case("lim", "flt_max", (130, 100, 32, 2), 47, False, (0, 0, 1352, 1346, 10, 7554)),
    Case("lim", "flt_max", (128, 128, 256, 64), 48, True, (0, 0, 1348, 1298, 411, 9927)),
    Case("lim", "zeros", (130, 128, 32, 2), 49, False, (0, 0, 0, 0, 0, 52204)),
    Case("lim", "zeros", (128, 100, 256, 64), 50, False, (0, 0, 0, 0, 0, 17165)),
    Case("xover", "flt_max", (130, 100, 2), 55, False, (0, 0, 13, 13, 31151, 0)),
    Case("xover", "flt_max", (130, 128, 4), 52, True, (0, 0, 29, 32, 84263, 0)),
    Case("xover", "zeros", (130, 100, 3), 53, False, (0, 0, 0, 0, 0, 38882)),
    Case("xover", "zeros", (130, 128, 2), 54, False, (0, 0, 0, 0, 0, 50044)),
]


def big(a):
    """Finite and above 2^127."""
    return np.isfinite(a) & (np.abs(a) > f32(2.0 ** 127))


def floats(out):
    return [a for a in out.values() if a.dtype == np.float32]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_cases_reach_the_edge(case):
    """The reference alone: it holds what the regime is named for, in the numbers the table pins."""
    ops, outs, state, _ = reference(case)
    got = counts(outs, state)
    print("%s: %d buffers; %s" % (case_id(case), len(outs), ", ".join("%d %s" % v for v in zip(got, COUNTS))))
    sub_out, sub_state, pinf, ninf, nan, negz = got
    plan, regime, T = case.plan, case.regime, case.shape[0]
    if regime in ("tail", "quiet"):
        assert sub_out > 0 and len(outs) <= TAIL_CAP + 3
        assert sub_state > 0 or regime == "quiet"                 # quiet: the smoothed gain sits at a few units
        assert pinf == ninf == nan == 0
    if regime == "flt_max":
        assert pinf > 0 and (ninf > 0 or plan == "meter")         # a meter's fields are magnitudes
        assert nan > 0 or plan in ("dyn", "resample")             # neither can make a NaN of finite samples
        # one buffer holds +inf, -inf and finite values above 2^127 side by side (the limiter: finite values that are
        # not zero; whatever it puts out that is finite is at or below its ceiling, and no ceiling is above 2^32)
        top = big if plan != "lim" else (lambda a: np.isfinite(a) & (a != 0))
        assert plan != "lim" or all((np.abs(o["y"][np.isfinite(o["y"])]) <= f32(2.0 ** 32)).all() for o in outs)
        assert any(any((a == np.inf).any() for a in floats(o)) and any(top(a).any() for a in floats(o))
                   and (plan == "meter" or any((a == -np.inf).any() for a in floats(o))) for o in outs)
    if regime == "flt_max" and any(op[0] == "reset" for op in ops):
        assert all(np.isfinite(a).all() for a in floats(outs[-1]))                   # after the reset: a new plan's
        fresh = HOSTS[plan](*case.shape)
        for op in ops:                                            # the tables in force, a new plan otherwise
            if op[0] in ("params", "gains", "delays", "decay", "splits"):
                getattr(fresh, op[0])(*(op[1:-1] + (False,) if op[0] in ("params", "gains") else op[1:]))
        last = [op for op in ops if op[0] == "run"][-1]
        assert differing([fresh.run(*last[1:])], outs[-1:]) == []
    if plan == "meter" and regime == "flt_max":
        flags = np.stack([o["rows"][:, 7] for o in outs])
        assert np.argwhere(flags != 0).tolist() == [[2, 64], [2, T - 1]]             # overflow inside is not flagged
        assert not np.isfinite(outs[0]["rows"][:, 2]).all() and not np.isfinite(outs[3]["rows"][:, 3]).all()
    if regime == "zeros":
        assert negz > 0 or plan in ("mix", "meter")               # the module's docstring says why
        assert pinf == ninf == nan == 0
    if regime.startswith("contain"):
        clean = reference(case, dirty=False)[1]
        assert all(np.isfinite(a).all() for o in clean for a in floats(o)) and nan > 0
        assert differing(outs[:1], clean[:1]) == []
        if plan == "delay":
            others = np.ones(T, bool)
            others[[64, T - 1]] = False
            assert all(same(o["y"][others], c["y"][others]) for o, c in zip(outs, clean))
            # Feedback 0 on track 64 does not let the NaN leave with its sample: w[n] = fmaf(0, NaN, x[n]) is a NaN, so
            # it goes round for good on both tracks, whatever the feedback
            assert all(not np.isfinite(o["y"][t]).all() for o in outs[1:5] for t in (64, T - 1))
            assert np.isfinite(outs[5]["y"]).all() and same(outs[5]["y"], clean[5]["y"])            # until reset
        else:
            assert differing(outs[2:], clean[2:]) == []           # a mix carries nothing
    assert got == case.want


def test_a_flushing_delay_line_is_caught_as_soon_as_a_subnormal_is_in_it():
    """The negative control: a twin whose line flushes subnormals to zero after every buffer, against the true twin on
    the tail cases.  The comparison the device is held to finds it at the first buffer behind a subnormal in the line."""
    for case in CASES:
        if (case.plan, case.regime) != ("delay", "tail"):
            continue
        ops, outs, state, _ = reference(case)
        true, flushed = HostDelay(*case.shape), FlushedDelay(*case.shape)
        first_sub = first_diff = None
        k = 0
        for op in ops:
            if op[0] != "run":
                getattr(true, op[0])(*op[1:]), getattr(flushed, op[0])(*op[1:])
                continue
            a, b = true.run(*op[1:]), flushed.run(*op[1:])
            if first_diff is None and not same(a["y"], b["y"]):
                first_diff = k
            if first_sub is None and subnormal(true.twin.line.hist).any():
                first_sub = k
            k += 1
        print("%s: the first subnormal enters the line in buffer %d, the outputs differ from buffer %d of %d"
              % (case_id(case), first_sub, first_diff, k))
        assert first_sub is not None and first_diff is not None and first_diff <= first_sub + 1
        assert differing([flushed.state()], [state]) != []


# ---- the strip's tail ------------------------------------------------------------------------------------------------
STRIP_SHAPE = (66, 100)
STRIP_SCALE = 2.0 ** -112                   # the schedule's seven buffers are too short for a full-scale tail to get there
STRIP_SUBNORMALS = {True: (18399, 12227), False: (12973, 9369)}


@functools.lru_cache(maxsize=None)
def strip_tail(scheduled=True):
    """The existing scenario with its first buffer alone, scaled down by a power of two, and silence behind it.
    scheduled: the whole schedule (160/147); else the tables of buffer 0 alone and 2/1, which a captured graph can
    replay.  Returns (the scenario, the composed restatement's outputs, the HostStrip afterwards)."""
    base = scenario(*STRIP_SHAPE) if scheduled else scenario(*STRIP_SHAPE, 2, 1)
    sc = types.SimpleNamespace(**vars(base))
    sc.xs, sc.keys = np.zeros_like(base.xs), np.zeros_like(base.keys)
    sc.xs[0], sc.keys[0] = base.xs[0] * f32(STRIP_SCALE), base.keys[0] * f32(STRIP_SCALE)
    sc.xs.setflags(write=False)
    sc.keys.setflags(write=False)
    strip = HostStrip(sc)
    if scheduled:
        got = strip.run()
    else:
        schedule(strip, sc, 0)
        outs = [strip.process(sc.xs[k], sc.keys[k]) for k in range(sc.n)]
        got = {name: np.stack([o[name] for o in outs]) for name in OUTPUTS}
        got["counts"] = [o["count"] for o in outs]
    return sc, got, strip


def strip_state(strip):
    m, bm, rv = strip.meter, strip.bus_meter, strip.reverb
    return [strip.eq.state, strip.bus_eq.state, strip.dyn.s, strip.delay.line.hist, rv.hist, rv.q, m.hist, m.hold,
            m.filter, m.ring, bm.hist, bm.hold, bm.filter, bm.ring, strip.resample.hist]


@pytest.mark.parametrize("scheduled", [True, False])
def test_the_strips_tail_reaches_the_subnormals(scheduled):
    sc, got, strip = strip_tail(scheduled)
    n_out = int(sum(subnormal(got[name]).sum() for name in OUTPUTS))
    n_state = int(sum(subnormal(a).sum() for a in strip_state(strip)))
    print("strip %dx%d, %s: %d subnormal output words, %d subnormal state words"
          % (STRIP_SHAPE + ("scheduled" if scheduled else "buffer 0's tables", n_out, n_state)))
    for name in OUTPUTS:
        assert np.isfinite(got[name]).all(), name
    assert n_out > 0 and n_state > 0
    assert (n_out, n_state) == STRIP_SUBNORMALS[scheduled]
