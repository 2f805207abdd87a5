"""The whole channel strip on the device (tests/strip_helpers.py): the nine plans one behind the other on one buffer, in
place where a strip runs in place, a buffer's launches and the buffers themselves queued without a host wait in between.

    a  against the composed restatement, bit for bit: every output of every buffer and every carried state
    b  each plan's process_batch between the schedule's points against per-buffer calls
    c  the strip captured into one graph on one stream: steady, and captured with ramps pending on all four ramped plans
    d  each plan captured alone, so that a failure of (c) names its plan (dynamics and reverb have theirs in their files)
    e  samples that are not finite stay where the header says

Every comparison is on bit patterns, two NaNs counting as the same.  (a) runs the equalisers in their ordered form, which
the restatement states to the bit; (b) to (e) are device against device with the equalisers in their default form, the
scan at bufsize 64.

What a captured launch bakes in (include/gab_c_api.h, "Captured calls") is the kernel form the host chose at the capture.
Captured with a ramp pending, dynamics, delay, reverb and mix replay the ramp form, which reads current, target and the
ramp table from the device and has the current := target copy behind it in the graph: the first replay is the ramp
buffer, later replays compute fmaf(target - current, r, current) with target - current = +0, the steady bits for every
table value but -0.0, and a set_*(ramp=True) between two replays is ramped in by the next one.  (c2) holds that.
"""
import numpy as np
import pytest

from plan_helpers import dev, gab, host  # noqa: F401 (gab: the fixture)
from strip_helpers import DeviceStrip, SHAPES, differing, reference, same, scenario, states_differing
from test_delay_host import delay_mix
from test_eq_host import eq_bank
from test_mix_host import gains

pytestmark = pytest.mark.gpu

IDS = ["%dx%d" % s for s in SHAPES]
LARGE = SHAPES[:2]
RAMPED = ("dyn", "delay", "reverb", "mix")


def sync():
    import torch
    torch.cuda.synchronize()


def check_against_the_restatement(strip, want, twin):
    """A DeviceStrip that has run the schedule against HostStrip.run()'s outputs and the HostStrip afterwards."""
    sync()
    assert differing(strip.outputs(), want) == []
    assert states_differing(strip, twin) == []


# ---- a. against the composed restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", SHAPES, ids=IDS)
def test_the_strip_against_the_composed_restatement(gab, T, B):
    sc = scenario(T, B)
    want, twin = reference(T, B)
    strip = DeviceStrip(gab, sc, sequential=True)
    assert strip.mix.form == sc.mix_form                       # the form the twin was given
    if (T, B) == SHAPES[0]:
        assert strip.mix.tracks > sc.mix_form[0] * sc.mix_form[1]            # more than one group
    strip.run()
    check_against_the_restatement(strip, want, twin)
    strip.close()


# ---- b. batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", LARGE, ids=IDS[:2])
def test_batches_between_the_schedule_points_are_per_buffer_calls(gab, T, B):
    sc = scenario(T, B)
    a, b = DeviceStrip(gab, sc), DeviceStrip(gab, sc)
    if B == 64:                                                # the scan form, on both
        assert a.eq.form != (0, 0) and a.bus_eq.form != (0, 0)
        for s in (a, b):
            assert all(t.data_ptr() % 16 == 0 and t[1].data_ptr() % 16 == 0 for t in (s.buf, s.bus))
    else:
        assert a.eq.form == (0, 0)
    a.run_batches()
    b.run()
    sync()
    assert differing(a.outputs(), b.outputs()) == []
    assert differing(a.states(), b.states()) == []
    assert a.counts == reference(T, B)[0]["counts"]
    for name in RAMPED:                                        # the ramp at the head of the second batch has run
        assert same(a.states()[name + ".current"], a.states()[name + ".target"])
    assert same(a.states()["mix.current"], sc.tables["gains1"])
    a.close()
    b.close()


# ---- c. the strip captured --------------------------------------------------------------------------------------
def capture(strip, k):
    """One graph of buffer k's launches, all on one side stream: (graph, the resampler's count)."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch = strip.prepare(k)
        with torch.cuda.graph(graph, stream=side):
            count = launch()
    torch.cuda.current_stream().wait_stream(side)
    sync()
    return graph, count


class Replayer:
    """Strip `a` replays one captured buffer slot with fresh inputs copied in; strip `b` makes plain calls."""

    def __init__(self, gab, sc, slot=1):
        self.sc, self.slot = sc, slot
        self.a, self.b = DeviceStrip(gab, sc), DeviceStrip(gab, sc)
        self.xs, self.keys = dev(sc.xs.reshape(sc.n, -1)), dev(sc.keys.reshape(sc.n, -1))
        self.graph = None

    def both(self, verb, *args):
        for s in (self.a, self.b):
            getattr(s, verb)(*args)

    def capture(self):
        before = self.a.states()
        self.graph, self.count = capture(self.a, self.slot)
        # the capture recorded launches without running them: every state is what it was
        assert differing(self.a.states(), before) == []

    def step(self, j):
        """Buffer j's inputs through the replay and through plain calls; the outputs agree."""
        self.a.buf[self.slot].copy_(self.xs[j])
        self.a.key[self.slot].copy_(self.keys[j])
        self.graph.replay()
        self.b.process(j)
        sync()
        assert differing(self.a.outputs(self.slot), self.b.outputs(j)) == [], j
        assert self.count == self.b.counts[-1] == 2 * self.sc.B

    def close(self):
        del self.graph
        self.a.close()
        self.b.close()


@pytest.mark.parametrize("T,B", LARGE, ids=IDS[:2])
def test_the_strip_captured_steady(gab, T, B):
    sc = scenario(T, B, 2, 1)
    r = Replayer(gab, sc)
    assert r.a.resample.period == 1
    for verb, args in (("eq_set", ("eq0", 0)), ("bus_eq_set", ("bus_eq0",)), ("dyn_set", ("dyn0", False)),
                       ("delay_set", ("delay0", False, 0)), ("reverb_delays", ("rev_delays0", 0)),
                       ("reverb_set", ("rev0", False)), ("mix_set", ("gains0", False))):
        r.both(verb, *args)
    r.both("process", 0)                                       # one buffer through plain calls
    r.capture()
    for j in range(1, 5):
        r.step(j)
    assert differing(r.a.states(), r.b.states()) == []
    # Captured with no ramp pending, the steady form reads `target` alone: tables set WITH a ramp behind the capture are
    # in force at the next replay, at once, as tables set without one are by a plain call; `current` is left behind.
    for verb, name, more in (("dyn_set", "dyn1", ()), ("delay_set", "delay1", (0,)), ("reverb_set", "rev1", ()),
                             ("mix_set", "gains1", ())):
        getattr(r.a, verb)(name, True, *more)
        getattr(r.b, verb)(name, False, *more)
    r.step(5)
    assert differing(r.a.states(), r.b.states()) == sorted(p + ".current" for p in RAMPED)
    r.close()


@pytest.mark.parametrize("T,B", LARGE, ids=IDS[:2])
def test_the_strip_captured_with_ramps_pending(gab, T, B):
    """Captured with a ramp pending on dynamics, delay, reverb and mix: the first replay is the ramp buffer, the second a
    steady one; new tables set with a ramp between two replays are ramped in by the next replay."""
    sc = scenario(T, B, 2, 1)
    r = Replayer(gab, sc)
    for verb, args in (("eq_set", ("eq0", 0)), ("bus_eq_set", ("bus_eq0",)), ("dyn_set", ("dyn0", False)),
                       ("delay_set", ("delay0", False, 0)), ("reverb_delays", ("rev_delays0", 0)),
                       ("reverb_set", ("rev0", False)), ("mix_set", ("gains0", False))):
        r.both(verb, *args)
    r.both("process", 0)

    def ramp_to(which):
        for verb, args in (("dyn_set", ("dyn" + which, True)), ("delay_set", ("delay" + which, True, 0)),
                           ("reverb_set", ("rev" + which, True)), ("mix_set", ("gains" + which, True))):
            r.both(verb, *args)

    def tables_are(which, current_too):
        st = r.a.states()
        for plan, name in zip(RAMPED, ("dyn", "delay", "rev", "gains")):
            assert same(st[plan + ".target"], sc.tables[name + which]), plan
            assert same(st[plan + ".current"], sc.tables[name + which]) == current_too, plan

    ramp_to("1")
    r.capture()
    tables_are("1", False)                                     # pending: current is still the old table
    r.step(1)                                                  # the ramp buffer
    tables_are("1", True)                                      # the copy behind it is in the graph
    r.step(2)                                                  # steady, in the ramp form
    ramp_to("0")
    tables_are("0", False)
    r.step(3)                                                  # ramped in by the next replay
    tables_are("0", True)
    r.step(4)
    assert differing(r.a.states(), r.b.states()) == []
    r.close()


# ---- d. each plan captured alone --------------------------------------------------------------------------------
T1 = 130


def _eq(gab, B):
    def make():
        plan = gab.EqPlan(T1, B, 3)
        plan.set_coeffs(dev(eq_bank(T1, 3, 5)))
        return plan
    return dict(make=make, n_in=T1 * B, n_out=T1 * B, prepare=lambda p, x, y: p.prepare(x, y),
                plain=lambda p, x, y: p.process(x, out=y), state=lambda p: [p.state()],
                check=lambda p: p.form != (0, 0) if B == 64 else p.form == (0, 0))


def _mix(gab, layout):
    B, M = 64, 3

    def make():
        plan = gab.MixPlan(2 * T1, B, M)
        plan.set_gains(dev(gains(2 * T1, M, 6)), ramp=False)
        return plan
    return dict(make=make, n_in=2 * T1 * B, n_out=M * B, prepare=lambda p, x, y: p.prepare(x, y, layout=layout),
                plain=lambda p, x, y: p.process(x, out=y, layout=layout), state=lambda p: list(p.gains()),
                check=lambda p: p.tracks > p.form[0] * p.form[1])


def _delay(gab, interp):
    B, md = 64, 168

    def make():
        plan = gab.DelayPlan(T1, B, md, interp)
        plan.set_params(dev(delay_mix(T1, B, md, interp, 1)), ramp=False)
        return plan
    return dict(make=make, n_in=T1 * B, n_out=T1 * B, prepare=lambda p, x, y: p.prepare(x, y),
                plain=lambda p, x, y: p.process(x, out=y), state=lambda p: list(p.line()) + list(p.params()),
                check=lambda p: True)


def _meter(gab):
    B = 64
    return dict(make=lambda: gab.MeterPlan(T1, B, 3), n_in=T1 * B, n_out=T1 * 8, prepare=lambda p, x, y: p.prepare(x, y),
                plain=lambda p, x, y: p.process(x, out=y), state=lambda p: list(p.state()), check=lambda p: True,
                host_only=lambda p: p.set_decay(0.5))          # a launch argument: the capture holds the old one


def _resample(gab):
    B = 64
    return dict(make=lambda: gab.ResamplePlan(T1, B, 2, 1), n_in=T1 * B, n_out=T1 * 2 * B, prepare=None,
                plain=lambda p, x, y: p.process(x, out=y), state=lambda p: [p.state()[0]],
                check=lambda p: p.period == 1 and p.out_capacity == 2 * B)


ALONE = {"eq-scan": lambda g: _eq(g, 64), "eq-ordered": lambda g: _eq(g, 100), "mix-track": lambda g: _mix(g, "track"),
         "mix-sample": lambda g: _mix(g, "sample"), "delay-linear": lambda g: _delay(g, "linear"),
         "delay-lagrange3": lambda g: _delay(g, "lagrange3"), "meter": _meter, "resample": _resample}


@pytest.mark.parametrize("which", list(ALONE))
def test_a_plan_captured_alone(gab, which):
    """One buffer by a plain call, the capture, three replays against plain calls on a second plan; states compared."""
    import torch
    c = ALONE[which](gab)
    a, b = c["make"](), c["make"]()
    assert c["check"](a)
    xs = dev(np.random.RandomState(7).uniform(-1.0, 1.0, (4, c["n_in"])).astype(np.float32))
    x, ya, yb = torch.empty(c["n_in"], device="cuda"), torch.full((c["n_out"],), 7.0, device="cuda"), torch.full((c["n_out"],), 7.0, device="cuda")
    assert x.data_ptr() % 16 == 0 and ya.data_ptr() % 16 == 0
    for p, y in ((a, ya), (b, yb)):
        c["plain"](p, xs[0], y)
    sync()
    assert same(host(ya), host(yb))
    before = [host(t) for t in c["state"](a)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = c["prepare"](a, x, ya) if c["prepare"] else None
        with torch.cuda.graph(graph, stream=side):
            if args is None:
                c["plain"](a, x, ya)
            else:
                a.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    sync()
    assert all(same(u, host(v)) for u, v in zip(before, c["state"](a)))       # recorded, not run
    for j in range(1, 4):
        x.copy_(xs[j])
        graph.replay()
        c["plain"](b, xs[j], yb)
        sync()
        assert same(host(ya), host(yb)), j
    assert all(same(host(u), host(v)) for u, v in zip(c["state"](a), c["state"](b)))
    if which == "resample":
        assert a.state()[1] == b.state()[1] == 0
    if "host_only" in c:
        # host state set behind the capture does not reach a replay (b never hears of it), and does reach a plain call
        c["host_only"](a)
        x.copy_(xs[0])
        graph.replay()
        c["plain"](b, xs[0], yb)
        sync()
        assert same(host(ya), host(yb))
        c["plain"](a, xs[1], ya)
        c["plain"](b, xs[1], yb)
        sync()
        assert not same(host(ya), host(yb))
    del graph
    a.close()
    b.close()


# ---- e. samples that are not finite -----------------------------------------------------------------------------
def test_nonfinite_samples_stay_where_the_header_says(gab):
    """A NaN in track 5 and an infinity in track 70 of buffer 1.  Equaliser, dynamics, delay and meter are per track (71 is
    70's link partner): no other track's buf or row moves by a bit.  The meter flags exactly the buffer the samples are
    in; a mix sums every track, so every bus is flagged."""
    T, B = SHAPES[0]
    sc = scenario(T, B)
    xs = sc.xs.copy()
    xs[1, 5, 17], xs[1, 70, 40] = np.nan, np.inf
    clean, dirty = DeviceStrip(gab, sc), DeviceStrip(gab, sc, xs=xs)
    clean.run()
    dirty.run()
    sync()
    c, d = clean.outputs(), dirty.outputs()
    others = np.ones(T, bool)
    others[[5, 70, 71]] = False
    assert same(c["buf"][:, others], d["buf"][:, others]) and same(c["track_rows"][:, others], d["track_rows"][:, others])
    assert same(c["gr"][:, others], d["gr"][:, others])
    assert same(c["buf"][0], d["buf"][0]) and same(c["bus"][0], d["bus"][0])             # and nothing before buffer 1
    flags = d["track_rows"][..., 7]
    assert set(np.unique(flags)) <= {0.0, 1.0}
    assert np.flatnonzero(flags[1]).tolist() == [5, 70] and not flags[0].any()
    assert not flags[:, others].any()                          # in later buffers on no other track
    assert not c["track_rows"][..., 7].any() and not c["bus_rows"][..., 7].any()
    assert (d["bus_rows"][1, :, 7] == 1.0).all() and not d["bus_rows"][0, :, 7].any()
    assert np.isfinite(d["buf"][:, others]).all() and not np.isfinite(d["buf"][1, 5]).all()
    clean.close()
    dirty.close()
