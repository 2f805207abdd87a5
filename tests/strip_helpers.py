"""A whole channel strip, on the host and on the device, driven through one schedule.  A plain module, as
plan_helpers.py is.

    HostStrip    the nine blocks as their restatements' twins (tests/test_*_host.py), composed.  It holds no arithmetic
                 of its own: every sample comes out of eq_reference_f32, dyn_reference_f32, delay_reference_f32, the
                 meter's, reverb's, mix's and resampler's twins.
    DeviceStrip  the real plans, every output preallocated for all the buffers and read after the last one; between the
                 launches of a buffer and between buffers nothing waits on the host but what a set_* call does itself
                 (every table is on the device before the first buffer).
    schedule     what happens before which buffer, written once and played on either.

The strip, per buffer k, every block track-major:

    buf <- x[k] [T][B];  EqPlan(T, B, 3) in place;  DynamicsPlan(T, B, link 2) in place, side chain key[k], meter gr[T];
    DelayPlan(T, B, max_delay, lagrange3) in place;  MeterPlan(T, B, window 3) reads buf -> track_rows[T][8];
    ReverbPlan(T, B, 4 lines, 2 outs) buf -> wet[2T][B];  MixPlan(2T, B, 3) wet -> bus[3][B];  EqPlan(3, B, 2) on bus in
    place;  MeterPlan(3, B, 1) reads bus -> bus_rows[3][8];  ResamplePlan(3, B, up, down) bus -> res[3][out_capacity].
"""
import functools
import types

import numpy as np

from plan_helpers import bits, dev, host
from test_delay_host import Twin as DelayTwin
from test_delay_host import capacity as delay_capacity
from test_delay_host import delay_mix
from test_dynamics_host import Twin as DynTwin
from test_dynamics_host import dyn_mix
from test_eq_host import eq_bank, eq_reference_f32
from test_meter_host import Twin as MeterTwin
from test_mix_host import Twin as MixTwin
from test_mix_host import gains
from test_resample_host import Twin as ResampleTwin
from test_reverb_host import MIN_DELAY as REVERB_MIN_DELAY
from test_reverb_host import Twin as ReverbTwin
from test_reverb_host import reverb_mix

# (tracks, bufsize): tracks across 64 and 128, one 64-sample chunk, the eq's scan form exists, 260 mix tracks (two
# groups); a short last chunk, no scan form, a multiple of 4; below every chunk and every vector width
SHAPES = [(130, 64), (66, 100), (6, 7)]
N_BUFFERS = 7
EQ_SECTIONS, BUS_EQ_SECTIONS, LINK, INTERP, TRACK_WINDOW, LINES, OUTS, BUSES = 3, 2, 2, "lagrange3", 3, 4, 2, 3
# k_mix.hip, mix_pick_form: up to 32 buses a leaf is 32 tracks and a group eight leaves.  The device tests hold
# plan.form to this.
MIX_FORM = (32, 8)
OUTPUTS = ("buf", "gr", "track_rows", "wet", "bus", "bus_rows", "res")


def same(a, b):
    """Bit for bit; two NaNs count as the same."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32:
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def levels(n, T, B, seed, lo, hi):
    """[n][T][B] noise at a level per track between 2^lo and 2^hi."""
    rng = np.random.RandomState(seed)
    scale = np.exp2(rng.uniform(lo, hi, (1, T, 1)))
    return (rng.uniform(-1.0, 1.0, (n, T, B)) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenario(T, B, up=160, down=147, n=N_BUFFERS, seed=0):
    """The tables, inputs and sizes of one strip; read only.  seed moves every table and every input."""
    sc = types.SimpleNamespace(T=T, B=B, up=up, down=down, n=n, seed=seed, mix_form=MIX_FORM)
    sc.max_delay = 2 * B + 40                                     # the delay plan's
    sc.reverb_max_delay = max(2 * B, REVERB_MIN_DELAY)            # reverb delays within [32, 2 B] (B = 7: all 32)
    rng = np.random.RandomState(1000 + seed)
    mid = slice(60, min(70, T))
    s = 10 * seed
    sc.tables = {
        "eq0": eq_bank(T, EQ_SECTIONS, 61 + s),
        "eq_mid": eq_bank(T, EQ_SECTIONS, 62 + s)[mid],           # tracks [60, 70), clipped to T: empty at T = 6
        "bus_eq0": eq_bank(BUSES, BUS_EQ_SECTIONS, 63 + s),
        "dyn0": dyn_mix(T, 1 + s), "dyn1": dyn_mix(T, 2 + s),
        "delay0": delay_mix(T, B, sc.max_delay, INTERP, 1 + s), "delay1": delay_mix(T, B, sc.max_delay, INTERP, 2 + s),
        "delay_tail": delay_mix(T, B, sc.max_delay, INTERP, 3 + s)[T - 2:],
        "rev0": reverb_mix(T, LINES, OUTS, 1 + s), "rev1": reverb_mix(T, LINES, OUTS, 2 + s),
        "rev_delays0": rng.randint(REVERB_MIN_DELAY, sc.reverb_max_delay + 1, (T, LINES)).astype(np.int32),
        "rev_delays_head": rng.randint(REVERB_MIN_DELAY, sc.reverb_max_delay + 1, (3, LINES)).astype(np.int32),
        "gains0": gains(OUTS * T, BUSES, 71 + s), "gains1": gains(OUTS * T, BUSES, 72 + s),
    }
    for name, t in sc.tables.items():
        if t.dtype == np.float32:
            assert not (np.signbit(t) & (t == 0)).any(), name     # no -0.0: fmaf(+0, r, -0) is +0, not the table's -0
        t.setflags(write=False)
    assert np.abs(np.concatenate([sc.tables[k][:, 1] for k in ("delay0", "delay1", "delay_tail")])).max() < 0.8
    sc.xs = levels(n, T, B, 2000 + seed, -3.0, 0.0)
    sc.keys = levels(n, T, B, 3000 + seed, -7.0, 1.0)             # below, around and above dyn_mix's thresholds
    sc.xs.setflags(write=False)
    sc.keys.setflags(write=False)
    return sc


def schedule(strip, sc, k):
    """What is set before buffer k, on a HostStrip or a DeviceStrip."""
    T = sc.T
    if k == 0:                                                    # every table at once
        strip.eq_set("eq0", 0)
        strip.bus_eq_set("bus_eq0")
        strip.dyn_set("dyn0", False)
        strip.delay_set("delay0", False, 0)
        strip.reverb_delays("rev_delays0", 0)
        strip.reverb_set("rev0", False)
        strip.mix_set("gains0", False)
    if k == 2:                                                    # a ramp on all four ramped plans together
        strip.dyn_set("dyn1", True)
        strip.delay_set("delay1", True, 0)
        strip.reverb_set("rev1", True)
        strip.mix_set("gains1", True)
        if sc.tables["eq_mid"].shape[0]:
            strip.eq_set("eq_mid", 60)
        strip.reverb_delays("rev_delays_head", 0)
    if k == 4:
        strip.delay_set("delay_tail", False, T - 2)
        strip.meter_decay(0.5)
    if k == 5:
        strip.delay_reset()
        strip.resample_reset()


SCHEDULE_POINTS = (0, 2, 4, 5)          # the buffers schedule() acts before


class EqTwin:
    """An equaliser plan's coefficients and carried state; process() is eq_reference_f32."""

    def __init__(self, T, S):
        self.coeffs = np.zeros((T, S, 5), np.float32)
        self.coeffs[..., 0] = 1.0
        self.state = np.zeros((T, S, 2), np.float32)

    def set_coeffs(self, c, first_track=0):
        self.coeffs[first_track:first_track + c.shape[0]] = c

    def process(self, x):
        return eq_reference_f32(x, self.coeffs, self.state)


class HostStrip:
    def __init__(self, sc):
        T, B = sc.T, sc.B
        self.sc = sc
        self.eq = EqTwin(T, EQ_SECTIONS)
        self.dyn = DynTwin(T, B, LINK)
        self.delay = DelayTwin(T, B, sc.max_delay, INTERP)
        self.meter = MeterTwin(T, B, TRACK_WINDOW)
        self.reverb = ReverbTwin(T, B, LINES, OUTS, sc.reverb_max_delay)
        self.mix = MixTwin(OUTS * T, B, BUSES, *sc.mix_form)
        self.bus_eq = EqTwin(BUSES, BUS_EQ_SECTIONS)
        self.bus_meter = MeterTwin(BUSES, B, 1)
        self.resample = ResampleTwin(BUSES, B, sc.up, sc.down)

    # ---- the schedule's verbs ----
    def eq_set(self, name, first):
        self.eq.set_coeffs(self.sc.tables[name], first)

    def bus_eq_set(self, name):
        self.bus_eq.set_coeffs(self.sc.tables[name])

    def dyn_set(self, name, ramp):
        self.dyn.set_params(self.sc.tables[name], ramp=ramp)

    def delay_set(self, name, ramp, first):
        self.delay.set_params(self.sc.tables[name], ramp=ramp, first_track=first)

    def reverb_set(self, name, ramp):
        self.reverb.set_params(self.sc.tables[name], ramp=ramp)

    def reverb_delays(self, name, first):
        self.reverb.set_delays(self.sc.tables[name], first_track=first)

    def mix_set(self, name, ramp):
        self.mix.set_gains(self.sc.tables[name], ramp=ramp)

    def meter_decay(self, decay):
        self.meter.set_decay(decay)

    def delay_reset(self):
        self.delay.reset()

    def resample_reset(self):
        self.resample.reset()

    def ramped(self):
        return (self.dyn, self.delay, self.reverb, self.mix)

    # ---- one buffer ----
    def wet_rows(self, buf):
        """Reverb's block as the mix takes it: row t * outs + o."""
        return self.reverb.process(buf)

    def front(self, x, key):
        buf = self.eq.process(x)
        buf, gr = self.dyn.process(buf, key)
        return self.delay.process(buf), gr

    def process(self, x, key):
        out = {}
        out["buf"], out["gr"] = self.front(x, key)
        out["track_rows"] = self.meter.process(out["buf"])
        out["wet"] = self.wet_rows(out["buf"])
        out["bus"] = self.bus_eq.process(self.mix.process(out["wet"]))
        out["bus_rows"] = self.bus_meter.process(out["bus"])
        out["res"], out["count"] = self.resample.process(out["bus"])
        return out

    def run(self, first=0, last=None, record=None):
        """Buffers [first, last) through the schedule; returns the outputs stacked, counts a list."""
        sc = self.sc
        last = sc.n if last is None else last
        outs = []
        for k in range(first, last):
            schedule(self, sc, k)
            if record is not None:
                record(self, k)
            outs.append(self.process(sc.xs[k], sc.keys[k]))
        got = {name: np.stack([o[name] for o in outs]) for name in OUTPUTS}
        got["counts"] = [o["count"] for o in outs]
        return got


@functools.lru_cache(maxsize=None)
def reference(T, B, up=160, down=147):
    """(the composed restatement's outputs over the schedule, the HostStrip afterwards); computed once, read only."""
    strip = HostStrip(scenario(T, B, up, down))
    got = strip.run()
    for name in OUTPUTS:
        got[name].setflags(write=False)
    return got, strip


class DeviceStrip:
    """The plans of one strip.  xs / keys: [n][T][B] inputs other than the scenario's."""

    def __init__(self, gab, sc, sequential=False, xs=None, keys=None):
        import torch
        T, B, n = sc.T, sc.B, sc.n
        self.sc, self.sequential = sc, sequential
        self.eq = gab.EqPlan(T, B, EQ_SECTIONS)
        self.dyn = gab.DynamicsPlan(T, B, LINK)
        self.delay = gab.DelayPlan(T, B, sc.max_delay, INTERP)
        self.meter = gab.MeterPlan(T, B, TRACK_WINDOW)
        self.reverb = gab.ReverbPlan(T, B, lines=LINES, outs=OUTS, max_delay=sc.reverb_max_delay)
        self.mix = gab.MixPlan(OUTS * T, B, BUSES)
        self.bus_eq = gab.EqPlan(BUSES, B, BUS_EQ_SECTIONS)
        self.bus_meter = gab.MeterPlan(BUSES, B, 1)
        self.resample = gab.ResamplePlan(BUSES, B, sc.up, sc.down)
        self.plans = (self.eq, self.dyn, self.delay, self.meter, self.reverb, self.mix, self.bus_eq, self.bus_meter,
                      self.resample)
        self.tables = {name: dev(t) for name, t in sc.tables.items() if t.size}
        OC = self.resample.out_capacity

        def block(*shape):
            return torch.full(shape, 7.0, device="cuda")
        self.buf = dev((sc.xs if xs is None else xs).reshape(n, T * B))          # processed in place
        self.key = dev((sc.keys if keys is None else keys).reshape(n, T * B))
        self.gr, self.track_rows, self.wet = block(n, T), block(n, T, 8), block(n, OUTS * T * B)
        self.bus, self.bus_rows, self.res = block(n, BUSES * B), block(n, BUSES, 8), block(n, BUSES, OC)
        self.counts = []
        torch.cuda.synchronize()

    def close(self):
        for p in self.plans:
            p.close()

    # ---- the schedule's verbs ----
    def eq_set(self, name, first):
        t = self.tables[name]
        self.eq.set_coeffs(t, first, t.shape[0])

    def bus_eq_set(self, name):
        self.bus_eq.set_coeffs(self.tables[name])

    def dyn_set(self, name, ramp):
        self.dyn.set_params(self.tables[name], ramp=ramp)

    def delay_set(self, name, ramp, first):
        self.delay.set_params(self.tables[name], ramp=ramp, first_track=first)

    def reverb_set(self, name, ramp):
        self.reverb.set_params(self.tables[name], ramp=ramp)

    def reverb_delays(self, name, first):
        self.reverb.set_delays(self.tables[name], first_track=first)

    def mix_set(self, name, ramp):
        self.mix.set_gains(self.tables[name], ramp=ramp)

    def meter_decay(self, decay):
        self.meter.set_decay(decay)

    def delay_reset(self):
        self.delay.reset()

    def resample_reset(self):
        self.resample.reset()

    # ---- the launches ----
    def process(self, k):
        """Buffer k: nine plain calls, nothing read back."""
        seq = self.sequential
        buf = self.buf[k]
        self.eq.process(buf, out=buf, sequential=seq)
        self.dyn.process(buf, key=self.key[k], out=buf, gr=self.gr[k])
        self.delay.process(buf, out=buf)
        self.meter.process(buf, out=self.track_rows[k])
        self.reverb.process(buf, out=self.wet[k])
        self.mix.process(self.wet[k], out=self.bus[k])
        self.bus_eq.process(self.bus[k], out=self.bus[k], sequential=seq)
        self.bus_meter.process(self.bus[k], out=self.bus_rows[k])
        self.counts.append(self.resample.process(self.bus[k], out=self.res[k])[1])

    def process_batch(self, a, b):
        """Buffers [a, b): each plan's process_batch over the blocks of all of them, plan after plan."""
        buf, bus = self.buf[a:b].view(-1), self.bus[a:b].view(-1)
        self.eq.process_batch(buf, out=buf)
        self.dyn.process_batch(buf, key=self.key[a:b].view(-1), out=buf, gr=self.gr[a:b].view(-1))
        self.delay.process_batch(buf, out=buf)
        self.meter.process_batch(buf, out=self.track_rows[a:b])
        self.reverb.process_batch(buf, out=self.wet[a:b].view(-1))
        self.mix.process_batch(self.wet[a:b].view(-1), out=bus)
        self.bus_eq.process_batch(bus, out=bus)
        self.bus_meter.process_batch(bus, out=self.bus_rows[a:b])
        self.counts += self.resample.process_batch(bus, out=self.res[a:b])[1]

    def prepare(self, k):
        """launch() for buffer k's blocks from prepare() / launch, and process(..., out=...) for the resampler which has
        no prepare: what a capture records.  Call it with the capturing stream current.  The equalisers take their
        default form."""
        buf, bus = self.buf[k], self.bus[k]
        args = [(self.eq, self.eq.prepare(buf, buf)),
                (self.dyn, self.dyn.prepare(buf, buf, key=self.key[k], gr=self.gr[k])),
                (self.delay, self.delay.prepare(buf, buf)),
                (self.meter, self.meter.prepare(buf, self.track_rows[k])),
                (self.reverb, self.reverb.prepare(buf, self.wet[k])),
                (self.mix, self.mix.prepare(self.wet[k], bus)),
                (self.bus_eq, self.bus_eq.prepare(bus, bus)),
                (self.bus_meter, self.bus_meter.prepare(bus, self.bus_rows[k]))]

        def launch():
            for plan, a in args:
                plan.launch(a)
            return self.resample.process(bus, out=self.res[k])[1]
        return launch

    def run(self):
        """Every buffer through the schedule by per-buffer calls; no host wait but a set_* call's own."""
        for k in range(self.sc.n):
            schedule(self, self.sc, k)
            self.process(k)

    def run_batches(self):
        """The same in batches between the schedule's points."""
        cuts = list(SCHEDULE_POINTS) + [self.sc.n]
        for a, b in zip(cuts, cuts[1:]):
            schedule(self, self.sc, a)
            self.process_batch(a, b)

    # ---- reading back ----
    def outputs(self, k=None):
        """Everything the strip wrote, as numpy, shaped like HostStrip.run()'s; k: buffer k alone."""
        sc = self.sc
        T, B = sc.T, sc.B
        sel = slice(None) if k is None else slice(k, k + 1)
        got = {"buf": host(self.buf[sel]).reshape(-1, T, B), "gr": host(self.gr[sel]),
               "track_rows": host(self.track_rows[sel]), "wet": host(self.wet[sel]).reshape(-1, OUTS * T, B),
               "bus": host(self.bus[sel]).reshape(-1, BUSES, B), "bus_rows": host(self.bus_rows[sel]),
               "res": host(self.res[sel])}
        if k is not None:
            got = {name: a[0].copy() for name, a in got.items()}
        else:
            got["counts"] = list(self.counts)
        return got

    def states(self):
        """{name: numpy} of every plan's carried state, whole: for a comparison of two DeviceStrips."""
        out = {"eq.state": host(self.eq.state()), "bus_eq.state": host(self.bus_eq.state()), "dyn.state": host(self.dyn.state())}
        for name, plan in (("dyn", self.dyn), ("delay", self.delay), ("reverb", self.reverb)):
            out[name + ".current"], out[name + ".target"] = (host(t) for t in plan.params())
        out["mix.current"], out["mix.target"] = (host(t) for t in self.mix.gains())
        out["delay.ring"], out["delay.pos"] = (host(t) for t in self.delay.line())
        for name, t in zip(("ring", "pos", "q", "delays"), self.reverb.state()):
            out["reverb." + name] = host(t)
        for which, plan in (("meter", self.meter), ("bus_meter", self.bus_meter)):
            for name, t in zip(("hist", "filter", "ring", "pos"), plan.state()):
                out[which + "." + name] = host(t)
        hist, k = self.resample.state()
        out["resample.hist"], out["resample.k"] = host(hist), np.array([k], np.int64)
        return out


def differing(a, b):
    """The names at which two {name: numpy} differ (bit for bit, two NaNs the same; lists by ==)."""
    assert set(a) == set(b)
    return [name for name in sorted(a)
            if not (a[name] == b[name] if isinstance(a[name], list) else same(a[name], b[name]))]


def states_differing(strip, twin):
    """The names of the carried states at which a DeviceStrip differs from a HostStrip."""
    st, bad = strip.states(), []

    def check(name, got, want):
        if not same(np.asarray(got), np.asarray(want)):
            bad.append(name)
    check("eq.state", st["eq.state"], twin.eq.state)
    check("bus_eq.state", st["bus_eq.state"], twin.bus_eq.state)
    check("dyn.state", st["dyn.state"], twin.dyn.s)
    for name, t in (("dyn", twin.dyn), ("delay", twin.delay), ("reverb", twin.reverb), ("mix", twin.mix)):
        check(name + ".current", st[name + ".current"], t.cur)
        check(name + ".target", st[name + ".target"], t.tgt)
    # the delay's ring: its newest max_delay + 3 values are the twin's, the positions its sample count
    line, ring = twin.delay.line, st["delay.ring"]
    cap = ring.shape[1]
    check("delay.capacity", np.int64(cap), np.int64(delay_capacity(twin.sc.B, twin.sc.max_delay)))
    check("delay.pos", st["delay.pos"], np.full(twin.sc.T, line.count % cap, np.int64))
    H = line.hist.shape[1]
    check("delay.ring", ring[:, (line.count - H + np.arange(H)) % cap], line.hist)
    # reverb: the newest max_delay words of every line, the positions, q and the delays
    rv, ring = twin.reverb, st["reverb.ring"]
    cap = ring.shape[2]
    check("reverb.capacity", np.int64(cap), np.int64(rv.cap))
    check("reverb.pos", st["reverb.pos"], np.full(twin.sc.T, rv.pos, np.int64))
    check("reverb.ring", ring[:, :, (rv.pos - rv.max_delay + np.arange(rv.max_delay)) & (cap - 1)], rv.hist)
    check("reverb.q", st["reverb.q"], rv.q)
    check("reverb.delays", st["reverb.delays"], rv.delays)
    for which, m in (("meter", twin.meter), ("bus_meter", twin.bus_meter)):
        hist = st[which + ".hist"]
        check(which + ".hist", hist[:, :11], m.hist)
        check(which + ".hold", hist[:, 11], m.hold)
        check(which + ".true_peak_max", hist[:, 12], m.tpmax)
        check(which + ".filter", st[which + ".filter"], m.filter)
        check(which + ".ring", st[which + ".ring"], m.ring)
        check(which + ".pos", st[which + ".pos"], np.full(m.T, m.pos, np.int64))
    check("resample.hist", st["resample.hist"], twin.resample.hist)
    check("resample.k", st["resample.k"], np.array([twin.resample.k], np.int64))
    return bad
