"""Eight bit-exact plans on the device at the edges of float32: tails that die through the subnormals, sums across
FLT_MAX, signed zeros, NaN and infinity containment, and one strip case.

Every case is a row of tests/test_edges_host.py's CASES.  Its tape of calls, recorded while the float32 twin ran it, is
replayed on the real plan; every buffer's outputs (meter rows, gain reduction and counts among them) and at the end every
carried state the plan exposes must be the twin's under same(): equal bits, two NaNs counting as equal whatever their
payload.  Each tape runs twice, by per-buffer calls and with every run of consecutive buffers as one process_batch; the
cases marked `offset` pass every block through a pointer 4 bytes off 16-byte alignment.  That the cases hold subnormals,
infinities, NaNs and -0.0 at all is established on the host (test_the_cases_reach_the_edge); nothing here asserts it.
"""
import types

import numpy as np
import pytest

import limiter_twin
import spectrum_twin as st
from plan_helpers import dev, gab, host  # noqa: F401 (gab: the fixture)
from strip_helpers import DeviceStrip, differing as strip_differing, same, schedule, states_differing
from test_delay_host import capacity as delay_capacity
from test_crossover_host import xover_first_refused
from test_edges_host import (CASES, HostSpec, case_id, delay_first_refused, differing, dyn_first_refused,
                             mix_first_refused, mix_form, play, reference, strip_tail)
from test_gate_host import gate_first_refused
from test_reverb_host import first_refused_param as reverb_first_refused

pytestmark = pytest.mark.gpu


def sync():
    import torch
    torch.cuda.synchronize()


class Blocks:
    """Device blocks, 16-byte aligned or (offset) 4 bytes past that."""

    def __init__(self, offset):
        self.offset = 1 if offset else 0

    def put(self, a, dtype=np.float32):
        import torch
        a = np.ascontiguousarray(a, dtype).ravel()
        big = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
        assert big.data_ptr() % 16 == 0
        t = big[self.offset:self.offset + a.size]
        t.copy_(torch.from_numpy(a.copy()))
        return t

    def blank(self, n):
        import torch
        big = torch.full((n + 4,), 7.0, device="cuda")
        return big[self.offset:self.offset + n]


class Dev:
    """What the device actors share: run() is a process call, run_batch() one process_batch over the buffers.
    inplace (where the header allows d_out == d_in): a process call writes over its input block."""

    inplace = False

    def __init__(self, gab, offset):
        self.gab, self.mem = gab, Blocks(offset)

    def run(self, x, key=None):
        return self.launch([x], [key], False)[0]

    def run_batch(self, xs, keys):
        return self.launch(xs, keys, True)

    def reset(self):
        self.p.reset()

    def params(self, p, ramp):
        self.p.set_params(dev(p), ramp=ramp)

    def params_tracks(self, p, first_track, ramp):
        self.p.set_params(dev(p), ramp=ramp, first_track=first_track)

    def named(self, i, first_track, width):
        """How the plan's refusal names value i of rows `width` wide (gab_plan.hpp, row_refusal)."""
        return "track %d field %d (" % (first_track + i // width, i % width)

    def refused(self, p, first_track, ramp):
        """The tape's refused set: refused here too, and the text names the value the host rule names."""
        i = self.rule(p)
        assert i is not None
        with pytest.raises(self.gab.GabError) as e:
            (self.gains_tracks if hasattr(self, "gains_tracks") else self.params_tracks)(p, first_track, ramp)
        assert e.value.code == -1 and self.named(i, first_track, p.shape[1]) in str(e.value), (str(e.value), i)

    def check(self, want):
        """The tape's check marker: the carried state here is the host actor's there.  (The windows of the delay and
        reverb rings are found from the recorded position.)"""
        sync()
        assert differing([self.state(self.twin_at(want))], [want]) == []
        self.checked = getattr(self, "checked", 0) + 1

    def twin_at(self, want):
        """What state() asks of the host actor, from a recorded state (the delay and reverb actors: where their rings
        stand)."""
        return None

    def close(self):
        self.p.close()


class DevMix(Dev):
    def __init__(self, gab, offset, T, B, M, layout="track"):
        Dev.__init__(self, gab, offset)
        self.p, self.shape, self.layout = gab.MixPlan(T, B, M), (M, B), layout
        assert self.p.form == mix_form(M)                          # the form the twin was given

    def gains(self, g, ramp):
        self.p.set_gains(dev(g), ramp=ramp)

    def gains_tracks(self, g, first_track, ramp):
        self.p.set_gains(dev(g), ramp=ramp, first_track=first_track)

    def rule(self, g):
        return mix_first_refused(g)

    def named(self, i, first_track, width):
        return "track %d bus %d is" % (first_track + i // width, i % width)

    def launch(self, xs, keys, batch):
        n, (M, B) = len(xs), self.shape
        xs = np.stack(xs)
        x = self.mem.put(xs.transpose(0, 2, 1) if self.layout == "sample" else xs)
        out = self.mem.blank(n * M * B)
        (self.p.process_batch if batch else self.p.process)(x, out=out, layout=self.layout)
        return [{"y": y} for y in host(out).reshape(n, M, B)]

    def state(self, twin):
        cur, tgt = self.p.gains()
        return {"current": host(cur), "target": host(tgt)}


class DevDelay(Dev):
    def __init__(self, gab, offset, T, B, M, interp):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.DelayPlan(T, B, M, interp), (T, B, M)

    def rule(self, p):
        return delay_first_refused(p, self.p.interp, self.p.max_delay)

    def twin_at(self, want):
        line = types.SimpleNamespace(count=int(want["pos"][0]), hist=want["line"])   # (the count mod the capacity)
        return types.SimpleNamespace(twin=types.SimpleNamespace(line=line))

    def launch(self, xs, keys, batch):
        n, (T, B, M) = len(xs), self.shape
        x = self.mem.put(np.stack(xs))
        out = x if self.inplace else self.mem.blank(n * T * B)
        (self.p.process_batch if batch else self.p.process)(x, out=out)
        return [{"y": y} for y in host(out).reshape(n, T, B)]

    def state(self, twin):
        T, B, M = self.shape
        (cur, tgt), (ring, pos) = self.p.params(), self.p.line()
        ring, line = host(ring), twin.twin.line
        cap, H = ring.shape[1], line.hist.shape[1]
        assert cap == delay_capacity(B, M)
        return {"current": host(cur), "target": host(tgt), "pos": host(pos),
                "line": ring[:, (line.count - H + np.arange(H)) % cap]}        # the newest max_delay + 3 words


class DevMeter(Dev):
    def __init__(self, gab, offset, T, B, W):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.MeterPlan(T, B, W), (T, B)

    def decay(self, v):
        self.p.set_decay(v)

    def launch(self, xs, keys, batch):
        n, (T, B) = len(xs), self.shape
        x, out = self.mem.put(np.stack(xs)), self.mem.blank(n * T * 8)
        (self.p.process_batch if batch else self.p.process)(x, out=out)
        return [{"rows": r} for r in host(out).reshape(n, T, 8)]

    def state(self, twin):
        hist, filt, ring, pos = (host(t) for t in self.p.state())
        assert not hist[:, 13:].any()
        return {"hist": hist[:, :11], "hold": hist[:, 11], "true_peak_max": hist[:, 12], "filter": filt, "ring": ring,
                "pos": pos}


class DevResample(Dev):
    def __init__(self, gab, offset, T, B, up, down, K):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.ResamplePlan(T, B, up, down, K), (T, B)
        assert self.p.ntaps == K

    def taps(self, t):
        self.p.set_taps(dev(t))

    def launch(self, xs, keys, batch):
        n, (T, B), OC = len(xs), self.shape, self.p.out_capacity
        x, out = self.mem.put(np.stack(xs)), self.mem.blank(n * T * OC)
        if batch:
            counts = self.p.process_batch(x, out=out)[1]
        else:
            counts = [self.p.process(x, out=out)[1]]
        return [{"y": y, "count": np.array([c], np.int64)} for y, c in zip(host(out).reshape(n, T, OC), counts)]

    def state(self, twin):
        hist, k = self.p.state()
        return {"hist": host(hist), "k": np.array([k], np.int64)}


class DevDyn(Dev):
    def __init__(self, gab, offset, T, B, link, keyed):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.DynamicsPlan(T, B, link), (T, B)

    def rule(self, p):
        return dyn_first_refused(p)

    def launch(self, xs, keys, batch):
        n, (T, B) = len(xs), self.shape
        assert all(k is None for k in keys) or all(k is not None for k in keys)
        x, gr = self.mem.put(np.stack(xs)), self.mem.blank(n * T)
        out = x if self.inplace else self.mem.blank(n * T * B)
        key = None if keys[0] is None else self.mem.put(np.stack(keys))
        (self.p.process_batch if batch else self.p.process)(x, key=key, out=out, gr=gr)
        return [{"y": y, "gr": g} for y, g in zip(host(out).reshape(n, T, B), host(gr).reshape(n, T))]

    def state(self, twin):
        cur, tgt = self.p.params()
        return {"current": host(cur), "target": host(tgt), "s": host(self.p.state())}


class DevReverb(Dev):
    def __init__(self, gab, offset, T, B, N, O, M):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.ReverbPlan(T, B, lines=N, outs=O, max_delay=M), (T, B, O, M)

    def delays(self, d):
        self.p.set_delays(dev(d))

    def delays_tracks(self, d, first_track):
        self.p.set_delays(dev(d), first_track=first_track)

    def rule(self, p):
        return reverb_first_refused(p, self.p.lines, self.shape[2])

    def twin_at(self, want):
        cap = 1
        while cap < self.shape[3] + 64:
            cap *= 2
        return types.SimpleNamespace(twin=types.SimpleNamespace(pos=int(want["pos"][0]), cap=cap))

    def launch(self, xs, keys, batch):
        n, (T, B, O, M) = len(xs), self.shape
        x = self.mem.put(np.stack(xs))
        assert O == 1 or not self.inplace
        out = x if self.inplace else self.mem.blank(n * T * O * B)
        (self.p.process_batch if batch else self.p.process)(x, out=out)
        return [{"y": y} for y in host(out).reshape(n, T * O, B)]

    def state(self, twin):
        T, B, O, M = self.shape
        (cur, tgt), (ring, pos, q, delays) = self.p.params(), self.p.state()
        ring, rv = host(ring), twin.twin
        cap = ring.shape[2]
        assert cap == rv.cap
        return {"current": host(cur), "target": host(tgt), "q": host(q), "pos": host(pos), "delays": host(delays),
                "lines": ring[:, :, (rv.pos - M + np.arange(M)) & (cap - 1)]}   # the newest max_delay words


class DevGate(Dev):
    def __init__(self, gab, offset, T, B, link, keyed):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.GatePlan(T, B, link), (T, B)

    def rule(self, p):
        return gate_first_refused(p)

    def launch(self, xs, keys, batch):
        import torch
        n, (T, B) = len(xs), self.shape
        assert all(k is None for k in keys) or all(k is not None for k in keys)
        x = self.mem.put(np.stack(xs))
        out = x if self.inplace else self.mem.blank(n * T * B)
        act = torch.full((n * T,), 7, dtype=torch.int32, device="cuda")
        key = None if keys[0] is None else self.mem.put(np.stack(keys))
        (self.p.process_batch if batch else self.p.process)(x, key=key, out=out, act=act)
        return [{"y": y, "act": a} for y, a in zip(host(out).reshape(n, T, B), host(act).reshape(n, T))]

    def state(self, twin):
        (cur, tgt), (g, c) = self.p.params(), self.p.state()
        return {"current": host(cur), "target": host(tgt), "gain": host(g), "count": host(c)}


class DevLim(Dev):
    def __init__(self, gab, offset, T, B, W, link):
        Dev.__init__(self, gab, offset)
        self.p, self.shape = gab.LimiterPlan(T, B, W, link), (T, B)
        assert self.p.latency == W - 1

    def rule(self, p):
        return limiter_twin.first_refused(p)

    def launch(self, xs, keys, batch):
        n, (T, B) = len(xs), self.shape
        x, gr = self.mem.put(np.stack(xs)), self.mem.blank(n * T)
        out = x if self.inplace else self.mem.blank(n * T * B)
        (self.p.process_batch if batch else self.p.process)(x, out=out, gr=gr)
        return [{"y": y, "gr": g} for y, g in zip(host(out).reshape(n, T, B), host(gr).reshape(n, T))]

    def state(self, twin):
        (cur, tgt), (xd, t, e) = self.p.params(), self.p.state()
        return {"current": host(cur), "target": host(tgt), "xd": host(xd), "t": host(t), "e": host(e)}


class DevXover(Dev):
    """Whether the plan has rows is not exposed: the actor keeps count of the sets that were accepted, and holds the
    plan to it by the refusal of process() for as long as there was none (a refused call launches nothing)."""

    NO_SPLITS = "no splits have been set: gab_xover_set_splits comes first"

    def __init__(self, gab, offset, T, B, K):
        Dev.__init__(self, gab, offset)
        self.p, self.shape, self.accepted = gab.CrossoverPlan(T, B, K), (T, B, K), 0

    def splits(self, rows):
        self.p.set_splits(dev(rows))
        self.accepted += 1

    def splits_tracks(self, rows, first_track):
        self.p.set_splits(dev(rows), first_track=first_track, n_tracks=rows.shape[0])
        self.accepted += 1

    def refused(self, rows, first_track):
        i, width = xover_first_refused(rows), 3 * (self.shape[2] - 1)
        assert i is not None
        with pytest.raises(self.gab.GabError) as e:
            self.p.set_splits(dev(rows), first_track=first_track)
        assert e.value.code == -1 and self.named(i, first_track, width) in str(e.value), (str(e.value), i)

    def unset_run(self, x):
        assert self.accepted == 0
        for batch in (False, True):
            with pytest.raises(self.gab.GabError) as e:
                self.launch([x], [None], batch)
            assert e.value.code == -1 and self.NO_SPLITS in str(e.value), str(e.value)

    def launch(self, xs, keys, batch):
        n, (T, B, K) = len(xs), self.shape
        x, out = self.mem.put(np.stack(xs)), self.mem.blank(n * K * T * B)
        (self.p.process_batch if batch else self.p.process)(x, out=out)
        return [{"bands": y} for y in host(out).reshape(n, K, T, B)]

    def state(self, twin):
        if not self.accepted:
            self.unset_run(np.zeros(self.shape[:2], np.float32))
        return {"state": host(self.p.state()), "rows": host(self.p.splits()),
                "has_rows": np.array([self.accepted > 0], np.int64)}


class DevSpec(Dev):
    """The transform is no bit twin, so the rows of a frame are held to a second device plan, `one`, of bufsize = hop =
    1024 with the window and edges in force: reset before every frame and given the frame's 1024 raw samples as the host
    actor holds them (history plus call), it must give the walked plan's rows bit for bit (a frame's bits depend only
    on its pair's windowed samples).  The framing is the host's, so an error in it cannot be on both sides.  The frame
    count of every call is exact.  `seen` keeps (raw samples, window, rows) of every frame for the accuracy bound."""

    def __init__(self, gab, offset, T, B, H, mode, bands):
        Dev.__init__(self, gab, offset)
        self.p, self.one = gab.SpectrumPlan(T, B, H, mode, bands), gab.SpectrumPlan(T, st.N, st.N, mode, bands)
        self.shape, self.bands, self.shadow, self.seen = (T, B, H), bands, HostSpec(T, B, H, mode, bands), []
        assert self.one.frames(1) == 1

    def window(self, w):
        for p in (self.p, self.one):
            p.set_window(dev(w))
        self.shadow.window(w)

    def edges(self, e):
        for p in (self.p, self.one):
            p.set_bands(e)
        self.shadow.edges(e)

    def refusal(self, call, text):
        with pytest.raises(self.gab.GabError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), str(e.value)

    def refused_window(self, w):
        k = st.bad_window(w)
        assert k is not None
        text = "the window's sum is zero" if k == "sum" else "window value %d is not finite" % k
        self.refusal(lambda: self.p.set_window(dev(w)), text + "; the plan keeps its window")

    def refused_edges(self, e):
        b = st.bad_edge(list(e), self.bands)
        assert b >= 0
        self.refusal(lambda: self.p.set_bands(e), "edge %d (%d) breaks 0 <= e_0 < e_1 < ... < e_bands <= 513; the plan "
                                                  "keeps its edges" % (b, e[b]))

    def reset(self):
        self.p.reset()
        self.shadow.reset()

    def launch(self, xs, keys, batch):
        n, (T, B, H) = len(xs), self.shape
        want = [self.shadow.run(x) for x in xs]                     # the host's counts and raw frames
        per_row = T * int(np.prod(self.p.row_shape))
        x, out = self.mem.put(np.stack(xs)), self.mem.blank(self.p.frames(n) * per_row)
        rows = (self.p.process_batch if batch else self.p.process)(x, out=out)
        F = rows.shape[0]
        counts = [int(w["count"][0]) for w in want]
        if not batch:
            counts = [F]                                             # (a batch returns one count: held as the sum)
        assert F == sum(counts), (F, counts)
        flat = host(out)
        assert (flat[F * per_row:] == 7.0).all()                     # rows past the count are not written
        got, raw = host(rows), np.concatenate([w["raw"] for w in want])
        assert raw.shape[0] == F
        for j in range(F):
            self.one.reset()
            single = self.one.process(self.mem.put(raw[j]))
            assert single.shape[0] == 1 and same(host(single)[0], got[j]), (len(self.seen), j)
            self.seen.append((raw[j], self.shadow.framer.w.copy(), got[j]))
        return [{"count": np.array([c], np.int64), "raw": w["raw"]} for c, w in zip(counts, want)]

    def state(self, twin):
        hist, w, p = self.p.state()
        return {"hist": host(hist), "window": host(w), "pos": np.array([p], np.int64)}

    def close(self):
        self.p.close()
        self.one.close()


DEVS = {"mix": DevMix, "delay": DevDelay, "meter": DevMeter, "resample": DevResample, "dyn": DevDyn, "reverb": DevReverb,
        "gate": DevGate, "lim": DevLim, "xover": DevXover, "spec": DevSpec}


def run_on_device(gab, case, ops, batch):
    """(outputs per buffer, the carried state at the end) of the tape on a new plan."""
    twin = reference(case)[3]
    actor = DEVS[case.plan](gab, case.offset, *case.shape)
    outs = play(ops, actor, batch=batch)
    sync()
    state = actor.state(twin)
    actor.close()
    return outs, state


# ---- a, b, c, d: every case against its twin -------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [False, True], ids=["per-buffer", "batched"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_plan_is_its_twin_at_the_edge(gab, case, batch):
    ops, want, want_state, _ = reference(case)
    got, state = run_on_device(gab, case, ops, batch)
    assert differing(got, want) == []
    assert differing([state], [want_state]) == []


# ---- d. containment: the clean run beside the dirty one ----------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c.regime.startswith("contain")], ids=case_id)
def test_a_nan_and_an_infinity_stay_where_the_twin_has_them(gab, case):
    """Mix: the buffers before the one that holds the samples are the clean run's (and so are those behind it: a mix
    carries nothing).  Delay: every other track's bits are the clean run's in every buffer.  The clean run is the clean
    twin's; the dirty run against the dirty twin is test_the_plan_is_its_twin_at_the_edge."""
    T = case.shape[0]
    ops_d, want_d, _, _ = reference(case)
    ops_c, want_c, state_c, _ = reference(case, dirty=False)
    dirty, _ = run_on_device(gab, case, ops_d, False)
    clean, state = run_on_device(gab, case, ops_c, False)
    assert differing(clean, want_c) == [] and differing([state], [state_c]) == []
    assert differing(dirty, want_d) == []
    if case.plan == "mix":
        assert differing(dirty[:1], clean[:1]) == [] and differing(dirty[2:], clean[2:]) == []
        assert not same(dirty[1]["y"], clean[1]["y"])
    else:
        others = np.ones(T, bool)
        others[[64, T - 1]] = False
        for k, (d, c) in enumerate(zip(dirty, clean)):
            assert same(d["y"][others], c["y"][others]), k
            assert np.array_equal(np.isfinite(d["y"]), np.isfinite(want_d[k]["y"])), k
        assert same(dirty[-1]["y"], clean[-1]["y"])                 # behind the reset


# ---- e. one strip case ---------------------------------------------------------------------------------------------
def test_the_strips_tail_plain(gab):
    """The existing schedule on one loud buffer and silence behind it, scaled so that the composed restatement walks into
    the subnormals within the schedule's seven buffers: every output and every carried state."""
    sc, want, twin = strip_tail(True)
    strip = DeviceStrip(gab, sc, sequential=True)
    assert strip.mix.form == sc.mix_form
    strip.run()
    sync()
    assert strip_differing(strip.outputs(), want) == []
    assert states_differing(strip, twin) == []
    strip.close()


def test_the_strips_tail_in_one_captured_graph(gab):
    """The same tail with buffer 0's tables alone at 2/1 (a captured resampler replays one position): buffer 0 by plain
    calls, then one graph of a buffer's nine launches replayed on the silence behind it."""
    import torch
    sc, want, twin = strip_tail(False)
    strip = DeviceStrip(gab, sc)
    assert strip.resample.period == 1 and strip.eq.form == (0, 0)       # bufsize 100: the ordered equaliser
    schedule(strip, sc, 0)
    strip.process(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        launch = strip.prepare(1)
        with torch.cuda.graph(graph, stream=side):
            count = launch()
    torch.cuda.current_stream().wait_stream(side)
    sync()
    xs, keys = dev(sc.xs.reshape(sc.n, -1)), dev(sc.keys.reshape(sc.n, -1))
    for k in range(1, sc.n):
        strip.buf[1].copy_(xs[k])
        strip.key[1].copy_(keys[k])
        graph.replay()
        sync()
        got = strip.outputs(1)
        bad = [name for name in sorted(got) if not same(got[name], want[name][k])]
        assert bad == [] and count == want["counts"][k], k
    assert states_differing(strip, twin) == []
    del graph
    strip.close()
