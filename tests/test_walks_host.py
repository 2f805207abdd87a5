"""The seeded walks of tests/walks.py without a GPU: every walk holds the orderings it is for, the host twins carry
their state exactly through them, and twins with one seeded defect each are told apart from the true ones by the very
comparison the device is held to (tests/test_walks_gpu.py): differing() on the outputs, same() on the state at every
check marker.  `pytest -s` prints every walk's census and, per control, the first buffer at which it is found.

The orderings (asserted from the tape alone, by walks.census): for the six plans with a ramped table, a range set
while another range's ramp is pending (an unramped one among them), a refused set and a reset while a ramp is pending,
two ramped sets before one buffer, a batch whose first buffer ramps, a ramp set between two batches; for every plan a
steady batch of three buffers or more and every call of the plan's vocabulary.  The meter plan and the resample plan
have no ramped table, nor have the crossover and the spectrum plan: the ramp conditions and the controls (a) to (d) do
not exist for them.  The limiter: ranges that cut a link group, and a cut behind a loud buffer at which the history of
needs holds a value below 1.  The crossover: the opening on a plan without rows before any whole set, a ranged set
across two owners, a set on a state that is not zero.  The spectrum plan: a reset off the hop grid, the three windows,
a batch of three buffers that emits no frame (bufsize 7 at hop 32) and one that emits more frames than it has buffers
(bufsize 1536 at hop 1000; bufsize 128 at hop 256 can do neither, bufsize 100 at hop 96 only by chance).

The controls, each a host actor with one defect:
    (a) the ramp runs through every buffer of a batch, not only the first          mix, delay, dyn, reverb, gate, lim
        (for the limiter this is (j); it must be found on a walk whose link groups take the launch in front)
    (b) an unramped range set clears `pending`                                     mix, delay, dyn, reverb, gate, lim
    (c) a refused set still commits `target`                                       mix, delay, dyn, reverb, gate, lim
    (d) reset leaves `current` behind `target`                                     mix, delay, dyn, reverb, gate, lim
    (e) the position wraps a buffer late: at period + 1, not at period             resample
    (f) the hold count is not carried across a call: an open gate restarts at H    gate
    (g) a ranged set on a new plan leaves zeros, not {1, 0, 0}, on the other rows  xover
    (h) a set clears the state                                                     xover
    (i) reset leaves the `e` history as it was                                     lim
    (k) reset keeps the position                                                   spec
    (l) set_window clears the history                                              spec
"""
import copy

import numpy as np
import pytest

import spectrum_twin as st
from test_edges_host import HOSTS, differing, play
from test_gate_host import HOLD
from walks import KEYED, MAX_BATCH, MAX_BUFFERS, RAMPED, WALKS, batches, census, owner_tracks, set_name, walk, walk_id

ORDERINGS = ("a range set on another range's pending ramp", "an unramped range set on another range's pending ramp",
             "a refused set on a pending ramp", "a reset on a pending ramp", "two ramped sets before a buffer",
             "a batch whose first buffer ramps", "a ramp set between two batches")


def vocabulary(plan):
    if plan in RAMPED:
        s = set_name(plan)
        v = ["run", "refused", "reset", "cut", "check"] + ["%s%s %s" % (s, t, r) for t in ("", "_tracks")
                                                           for r in ("ramped", "unramped")]
        return v + (["delays", "delays_tracks"] if plan == "reverb" else [])
    if plan == "xover":
        return ["run", "unset_run", "splits", "splits_tracks", "refused", "reset", "cut", "check"]
    if plan == "spec":
        return ["run", "window", "refused_window", "reset", "cut", "check"]
    return ["run", "decay" if plan == "meter" else "taps", "reset", "cut", "check"]


def checks(ops):
    return [op[1] for op in ops if op[0] == "check"]


def buffers_before_check(ops, n):
    """How many buffers lie before the n-th check marker."""
    seen = runs = 0
    for op in ops:
        if op[0] == "check":
            if seen == n:
                return runs
            seen += 1
        runs += op[0] == "run"
    return runs


# ---- the table -------------------------------------------------------------------------------------------------------
def test_the_table_of_walks_has_the_shapes_every_plan_needs():
    plans = sorted({w.plan for w in WALKS})
    assert plans == sorted(HOSTS) and len(WALKS) == 4 * len(plans) and len({w.seed for w in WALKS}) == len(WALKS)
    for plan in plans:
        ws = [w for w in WALKS if w.plan == plan]
        assert len(ws) == 4 and all(w.shape[0] <= 130 and 30 <= w.steps <= 50 for w in ws)
        # a buffer of a walk is at most 130 x 200 samples; only the spectrum plan, whose calls must be longer than its
        # history of 1023 samples once, spends that on two long tracks
        assert all(w.shape[1] <= 200 or (plan == "spec" and w.shape[0] * w.shape[1] <= 130 * 200) for w in ws)
        lanes = [w.shape[0] * (w.shape[2] if plan == "reverb" else 1) for w in ws]
        if plan == "spec":       # a workgroup owns 8 tracks and a wave a pair: a count that ends inside each, one within
            assert any(n > 8 and n % 8 and n % 2 for n in lanes) and any(n <= 8 for n in lanes)
        else:
            assert any(n > 64 and n % 64 for n in lanes) and any(w.shape[0] <= 64 for w in ws)
        assert {100, 128, 7} <= {w.shape[1] for w in ws}
    assert 130 in {w.shape[0] for w in WALKS if w.plan != "reverb"}
    assert {w.shape[2:] for w in WALKS if w.plan == "reverb"} >= {(4, 2, 64), (16, 1, 64)}
    assert {w.shape[2] for w in WALKS if w.plan == "gate"} == {1, 4, 16, 64}
    assert {w.shape[2] for w in WALKS if w.plan == "dyn"} == {1, 2}
    assert {w.shape[3] for w in WALKS if w.plan == "lim"} == {2, 8, 16, 64}
    assert {w.shape[2] for w in WALKS if w.plan == "lim"} >= {32, 128, 256}     # k <= 6, 7 and 8: the three ring shapes
    assert any(w.shape[1] < w.shape[2] - 1 for w in WALKS if w.plan == "lim")    # buffers shorter than W - 1
    assert {w.shape[2] for w in WALKS if w.plan == "xover"} == {2, 3, 4}
    assert {w.shape[3] for w in WALKS if w.plan == "spec"} == {"complex", "power"}
    assert {bool(w.shape[4]) for w in WALKS if w.plan == "spec"} == {True, False}
    spec = [w.shape[1:3] for w in WALKS if w.plan == "spec"]
    assert any(3 * B < H for B, H in spec) and any(B > st.HIST and 2 * B >= 3 * H for B, H in spec)
    assert {w.shape[3] for w in WALKS if w.plan == "delay"} == {"linear", "lagrange3"}
    assert {w.shape[2:] for w in WALKS if w.plan == "mix"} >= {(2, "track"), (33, "sample"), (33, "track"), (2, "sample")}
    assert {w.shape[2:4] for w in WALKS if w.plan == "resample"} >= {(2, 5), (1, 1024)}
    for plan in KEYED:
        assert {w.shape[3] for w in WALKS if w.plan == plan} == {True, False}


# ---- every walk has what it needs --------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WALKS, ids=walk_id)
def test_every_walk_has_what_it_needs(w):
    ops, outs, state, _ = walk(*w)
    c = census(w, ops)
    print("%s: %s" % (walk_id(w), ", ".join("%s %d" % kv for kv in sorted(c.items()))))
    assert len(outs) == c["run"] <= MAX_BUFFERS and 30 <= len(ops) - c["check"] <= w.steps + 8
    for name in vocabulary(w.plan):
        assert c.get(name, 0) > 0, name
    sizes = [n for _, n in batches(ops)]
    assert min(sizes) == 1 and max(sizes) <= MAX_BATCH and c.get("a steady batch of three or more", 0) > 0
    # a check behind every set, refused set and reset, and one at the end
    for i, op in enumerate(ops):
        if op[0] not in ("run", "cut", "check"):
            assert ops[i + 1][0] == "check", (i, op[0])
    assert ops[-1][0] == "check" and differing([ops[-1][1]], [state]) == []
    if w.plan in RAMPED:
        for name in ORDERINGS:
            assert c.get(name, 0) > 0, name
        T, own = w.shape[0], owner_tracks(w.plan, w.shape)
        ranges = [(op[2], op[2] + op[1].shape[0]) for op in ops if op[0].endswith("_tracks") or op[0] == "refused"]
        assert any(a % own and b % own and a // own == (b - 1) // own for a, b in ranges)        # inside one owner
        assert T <= own + 1 or any(a % own and b % own and a // own + 1 == (b - 1) // own for a, b in ranges)
        keyed = [op[2] is not None for op in ops if op[0] == "run"]
        assert (any(keyed) and not all(keyed)) if w.plan in KEYED and w.shape[3] else not any(keyed)
    if w.plan == "lim":
        link, W = w.shape[3], w.shape[2]
        assert c.get("a range that starts or ends inside a link group", 0) > 0
        fresh, held = HOSTS["lim"](*w.shape), 0
        for i, op in enumerate(ops):
            getattr(fresh, op[0])(*op[1:])
            if op[0] == "cut" and ops[i - 1][0] == "run" and ops[i + 1][0] == "run":
                held += int((fresh.twin.hist[1] < 1.0).any())
        gr = np.stack([o["gr"] for o in outs])
        print("    cuts at which the history of needs holds a value below 1: %d; gr < 1 on %d of %d rows"
              % (held, (gr < 1.0).sum(), gr.size))
        assert held > 0 and (gr < 1.0).any() and (gr == 1.0).any()
    if w.plan == "xover":
        assert c["the opening on a plan without rows"] == 1
        assert w.shape[0] <= owner_tracks(w.plan, w.shape) + 1 or c["a ranged set across two owners"] > 0
        fresh, moving = HOSTS["xover"](*w.shape), 0
        for op in ops:
            if op[0] in ("splits", "splits_tracks"):
                moving += bool(fresh.twin.state.any())
            getattr(fresh, op[0])(*op[1:])
        print("    sets that arrived on a state that was not zero: %d" % moving)
        assert moving > 0
    if w.plan == "spec":
        B, H, bands = w.shape[1], w.shape[2], w.shape[4]
        for name in ("a reset off the hop grid", "a hann window", "a positive window", "a one-hot window"):
            assert c.get(name, 0) > 0, name
        assert not bands or (c.get("edges", 0) > 0 and c.get("refused_edges", 0) > 0)
        assert 3 * B >= H or c["a batch of three or more that emits no frame"] > 0
        assert 2 * B < 3 * H or c["a batch that emits more frames than buffers"] > 0
        counts = [int(o["count"][0]) for o in outs]
        print("    frames per buffer %s" % counts)
        assert any(counts) and (3 * B >= H or counts.count(0) > len(counts) // 2)
    if w.plan == "gate":
        act = np.stack([o["act"] for o in outs])
        assert 0 < act.sum() < act.size * w.shape[1]
        fresh, carried = HOSTS["gate"](*w.shape), 0
        for i, op in enumerate(ops):
            getattr(fresh, op[0])(*op[1:])
            if op[0] == "cut" and ops[i - 1][0] == "run" and ops[i + 1][0] == "run":
                t = fresh.twin
                carried += int(((t.c >= 0) & (t.c < t.tgt[:, HOLD]) & (t.tgt[:, HOLD] > w.shape[1])).sum())
        print("    counts of a hold longer than the buffer carried across a cut: %d" % carried)
        assert carried > 0
    if w.plan == "resample":
        period = HOSTS["resample"](*w.shape).twin.period
        assert c.get("period - 1 -> 0 inside a batch", 0) > 0 and c["buffers behind a reset, at most"] >= period + 2
        counts = [int(o["count"][0]) for o in outs]
        print("    period %d, outputs per buffer %s" % (period, counts))
        assert any(counts) and (w.shape[2:4] != (1, 1024) or counts.count(0) >= 3 * (len(counts) // 4))


# ---- the twins carry their state through the walks -----------------------------------------------------------------
@pytest.mark.parametrize("w", WALKS, ids=walk_id)
def test_the_twin_in_batches_is_the_twin_in_single_calls(w):
    """play() with the cut and check markers, on a new host actor whose batch is its buffers one by one: the outputs
    and the state at every check are the tape's own."""
    ops, outs, _, _ = walk(*w)
    for batch in (False, True):
        actor = HOSTS[w.plan](*w.shape)
        assert differing(play(ops, actor, batch=batch), outs) == []
        assert differing(actor.checks, checks(ops)) == []


@pytest.mark.parametrize("w", WALKS, ids=walk_id)
def test_cut_and_resume(w):
    """A deep copy of the host actor taken at a random check goes on alone: bit for bit the uninterrupted run."""
    ops, outs, state, _ = walk(*w)
    marks = [i for i, op in enumerate(ops) if op[0] == "check"][:-1]
    at = marks[int(np.random.RandomState(w.seed).randint(len(marks)))]
    actor = HOSTS[w.plan](*w.shape)
    head = play(ops[:at + 1], actor)
    resumed = copy.deepcopy(actor)
    tail = play(ops[at + 1:], resumed)
    assert len(tail) > 0 and differing(head + tail, outs) == []
    assert differing([resumed.state()], [state]) == []
    assert differing(resumed.checks, checks(ops)) == []


# ---- the negative controls -------------------------------------------------------------------------------------------
def ramp_through_the_batch(base):
    class Control(base):
        def run_batch(self, xs, keys):
            t = self.twin
            if not t.pending:
                return base.run_batch(self, xs, keys)
            cur, outs = t.cur.copy(), []
            for x, k in zip(xs, keys):
                t.cur[:], t.pending = cur, True
                outs.append(self.run(x, k))
            return outs
    return Control


def unramped_range_clears_pending(base):
    class Control(base):
        def params_tracks(self, p, first_track, ramp):
            base.params_tracks(self, p, first_track, ramp)
            self.twin.pending = self.twin.pending and ramp

        def gains_tracks(self, g, first_track, ramp):
            base.gains_tracks(self, g, first_track, ramp)
            self.twin.pending = self.twin.pending and ramp
    return Control


def refused_commits_target(base):
    class Control(base):
        def refused(self, p, first_track, ramp):
            base.refused(self, p, first_track, ramp)
            self.twin.tgt[first_track:first_track + p.shape[0]] = p
    return Control


def reset_leaves_current(base):
    class Control(base):
        def reset(self):
            cur = self.twin.cur.copy()
            base.reset(self)
            self.twin.cur[:] = cur
    return Control


def position_wraps_a_buffer_late(base):
    class Control(base):
        late = 0

        def reset(self):
            base.reset(self)
            self.late = 0

        def run(self, x, key=None):
            self.twin.k = self.late                                  # the twin works in exact integers from any k
            self.late = (self.late + 1) % (self.twin.period + 1)
            return base.run(self, x, key)
    return Control


def hold_restarts_at_a_call(base):
    class Control(base):
        def run(self, x, key=None):
            t = self.twin
            t.c = np.where(t.c >= 0, t.tgt[:, HOLD].astype(np.int32), t.c).astype(np.int32)
            return base.run(self, x, key)
    return Control


def ranged_set_on_a_new_plan_leaves_zeros(base):
    class Control(base):
        def splits_tracks(self, rows, first_track):
            new = self.twin.rows is None
            base.splits_tracks(self, rows, first_track)
            if new:
                keep = self.twin.rows[first_track:first_track + len(rows)].copy()
                self.twin.rows[:] = 0.0
                self.twin.rows[first_track:first_track + len(rows)] = keep
    return Control


def set_clears_the_state(base):
    class Control(base):
        def splits(self, rows):
            base.splits(self, rows)
            self.twin.reset()

        def splits_tracks(self, rows, first_track):
            base.splits_tracks(self, rows, first_track)
            self.twin.reset()
    return Control


def reset_leaves_the_e_history(base):
    class Control(base):
        def reset(self):
            e = self.twin.hist[2].copy()
            base.reset(self)
            self.twin.hist = self.twin.hist[:2] + (e,)
    return Control


def reset_keeps_the_position(base):
    class Control(base):
        def reset(self):
            p = self.framer.p
            base.reset(self)
            self.framer.p = p
    return Control


def set_window_clears_the_history(base):
    class Control(base):
        def window(self, w):
            base.window(self, w)
            self.framer.hist[:] = 0.0
    return Control


CONTROLS = {"a: the ramp runs through every buffer of a batch": (ramp_through_the_batch, RAMPED),
            "b: an unramped range set clears pending": (unramped_range_clears_pending, RAMPED),
            "c: a refused set commits target": (refused_commits_target, RAMPED),
            "d: reset leaves current behind target": (reset_leaves_current, RAMPED),
            "e: the position wraps a buffer late": (position_wraps_a_buffer_late, ("resample",)),
            "f: the hold count restarts at a call": (hold_restarts_at_a_call, ("gate",)),
            "g: a ranged set on a new plan leaves zeros": (ranged_set_on_a_new_plan_leaves_zeros, ("xover",)),
            "h: a set clears the state": (set_clears_the_state, ("xover",)),
            "i: reset leaves the e history": (reset_leaves_the_e_history, ("lim",)),
            "k: reset keeps the position": (reset_keeps_the_position, ("spec",)),
            "l: set_window clears the history": (set_window_clears_the_history, ("spec",))}


@pytest.mark.parametrize("plan,name", [(p, n) for n in sorted(CONTROLS) for p in CONTROLS[n][1]])
def test_the_walks_tell_a_control_from_the_true_twin(plan, name):
    """Replayed in batches, as the device replays them.  Found on the outputs: the first buffer that differs; found on
    the state alone: the check marker, and how many buffers lie before it."""
    found, wide = 0, 0
    for w in WALKS:
        if w.plan != plan:
            continue
        ops, outs, _, _ = walk(*w)
        control = CONTROLS[name][0](HOSTS[plan])(*w.shape)
        try:
            with np.errstate(invalid="ignore", over="ignore"):
                got = play(ops, control, batch=True)
        except AssertionError:                                       # a twin that asserts on its own tables (a NaN delay)
            got = None
        seen = control.checks
        out_diff = differing(got, outs) if got is not None else []
        state_diff = differing(seen, checks(ops)[:len(seen)])
        where = [] if got is not None else ["the twin refuses to go on behind check %d" % (len(seen) - 1)]
        if out_diff:
            where.append("outputs from buffer %d (%s)" % out_diff[0])
        if state_diff:
            n, field = state_diff[0]
            where.append("state from check %d (%s), behind %d buffers" % (n, field, buffers_before_check(ops, n)))
        print("%s, %s: %s" % (name, walk_id(w), "; ".join(where) or "not found"))
        found += bool(out_diff or state_diff or got is None)
        wide += bool(out_diff or state_diff) and plan == "lim" and w.shape[3] >= 16
    assert found > 0
    if plan == "lim" and name.startswith("a:"):                      # (j): also where the detector launch runs in front
        assert wide > 0
