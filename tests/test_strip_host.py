"""The composed restatement of the channel strip (tests/strip_helpers.py) without a GPU: that it is no vacuous
yardstick.  On the twin alone, at every shape of tests/test_strip_gpu.py and for the committed seeds: the compressor
compresses on most tracks and rests on some, every delay line is heard and most feed back, every bus carries signal,
everything is finite, the resampler's counts take both of their values, the meter's rows move; the buffer behind the ramp
buffer is a steady one; and the strip cut in the middle and resumed from a copy of its twins gives the same bits, so the
twins' state machines compose."""
import copy

import numpy as np
import pytest

from strip_helpers import N_BUFFERS, OUTPUTS, SHAPES, HostStrip, differing, reference, same, scenario

IDS = ["%dx%d" % s for s in SHAPES]


@pytest.mark.parametrize("T,B", SHAPES, ids=IDS)
def test_the_scenario_exercises_every_block(T, B):
    sc = scenario(T, B)
    got, _ = reference(T, B)
    gr = got["gr"]
    assert ((gr < 0).sum(axis=1) >= T / 2).any(), (gr < 0).sum(axis=1)       # compressing on half the tracks or more
    assert (gr == 0).any() and (gr <= 0).all()                                 # and at rest on some
    for name in ("delay0", "delay1"):
        p = sc.tables[name]
        assert (p[:, 2] != 0).all() and (p[:, 1] != 0).sum() >= T / 2, name    # wet everywhere, feedback on half
    assert (got["bus_rows"][1:, :, 0] > 0).all()                               # every bus has a peak from buffer 1 on
    for name in OUTPUTS:
        assert np.isfinite(got[name]).all(), name
    assert not got["track_rows"][..., 7].any() and not got["bus_rows"][..., 7].any()
    L, M = sc.up, sc.down
    floor, ceil = (B * L) // M, -(-(B * L) // M)
    since_reset = [k if k < 5 else k - 5 for k in range(N_BUFFERS)]           # resample.reset() before buffer 5
    want = [-(-((k + 1) * B * L) // M) - -(-(k * B * L) // M) for k in since_reset]
    assert got["counts"] == want and set(want) <= {floor, ceil}
    if B == 100:
        # 100 * 160 / 147 = 108.84: the first floor is the seventh buffer behind a reset, and the schedule resets before
        # buffer 5, so this shape sees the ceiling alone; the other two see both
        assert set(want) == {ceil} and -(-(7 * B * L) // M) - -(-(6 * B * L) // M) == floor
    else:
        assert set(want) == {floor, ceil}, want                                # the floor and the ceiling
    for k, n_out in enumerate(got["counts"]):                                  # samples, then the zero fill
        assert got["res"][k, :, :n_out].any(axis=1).all() and not got["res"][k, :, n_out:].any()
    rows = got["track_rows"]
    for f in (0, 1, 2, 3, 6):                                                  # the rows move with the track and the buffer
        assert len(np.unique(rows[0, :, f])) == T and len(np.unique(rows[:, 0, f])) == N_BUFFERS, f
    assert (got["wet"][:, 0::2] != got["wet"][:, 1::2]).any()                  # reverb's two outputs differ


@pytest.mark.parametrize("T,B", SHAPES, ids=IDS)
def test_the_schedule_reaches_the_twins(T, B):
    """What schedule() does is seen in the twins' state before and behind the buffers it names."""
    sc = scenario(T, B)
    seen = {}

    def record(strip, k):
        seen[k] = (tuple(t.pending for t in strip.ramped()), strip.delay.line.count, strip.resample.k,
                   float(strip.meter.decay), strip.delay.tgt.copy(), strip.eq.coeffs.copy(), strip.reverb.delays.copy())
    strip = HostStrip(sc)
    strip.run(record=record)
    for k in range(N_BUFFERS):
        assert seen[k][0] == ((True,) * 4 if k == 2 else (False,) * 4), k      # pending in front of buffer 2 alone
    assert all(same(t.cur, t.tgt) for t in strip.ramped())
    assert [seen[k][1] for k in range(N_BUFFERS)] == [0, B, 2 * B, 3 * B, 4 * B, 0, B]          # delay.reset before 5
    assert seen[5][2] == 0 and seen[4][3] == 0.5 and seen[3][3] == 1.0
    assert same(seen[4][4][T - 2:], sc.tables["delay_tail"]) and same(seen[4][4][:T - 2], sc.tables["delay1"][:T - 2])
    assert not same(seen[4][4][T - 2:], seen[3][4][T - 2:])
    if T > 60:
        assert same(seen[2][5][60:70], sc.tables["eq_mid"]) and same(seen[2][5][:60], sc.tables["eq0"][:60])
        assert not same(seen[2][5], seen[1][5])
    assert same(seen[2][6][:3], sc.tables["rev_delays_head"]) and same(seen[2][6][3:], sc.tables["rev_delays0"][3:])


@pytest.mark.parametrize("T,B", SHAPES, ids=IDS)
def test_the_buffer_behind_the_ramp_buffer_is_steady(T, B):
    """Behind buffer 2 no ramp is pending and current == target on all four ramped twins; and buffer 3 run in the ramp
    form from there (target - current is +0, and fmaf(+0, r, c) == c for every c but -0, which no table holds) gives the
    bits of the steady form: what a captured ramp-form launch replays."""
    sc = scenario(T, B)
    got, _ = reference(T, B)
    strip = HostStrip(sc)
    strip.run(0, 3)
    assert not any(t.pending for t in strip.ramped())
    for t, name in zip(strip.ramped(), ("dyn1", "delay1", "rev1", "gains1")):
        assert same(t.cur, t.tgt) and same(t.tgt, sc.tables[name]), name
    again = copy.deepcopy(strip)
    for t in again.ramped():
        t.pending = True
    ramp_form = again.process(sc.xs[3], sc.keys[3])
    steady = strip.process(sc.xs[3], sc.keys[3])
    for name in OUTPUTS:
        assert same(ramp_form[name], steady[name]) and same(steady[name], got[name][3]), name
    # and the ramp buffer itself is no steady buffer of either table
    head = HostStrip(sc)
    head.run(0, 2)
    for ramp in (True, False):
        other = copy.deepcopy(head)
        for name, set_ in (("dyn1", other.dyn_set), ("rev1", other.reverb_set), ("gains1", other.mix_set)):
            set_(name, ramp)
        other.delay_set("delay1", ramp, 0)
        if sc.tables["eq_mid"].shape[0]:
            other.eq_set("eq_mid", 60)
        other.reverb_delays("rev_delays_head", 0)
        out = other.process(sc.xs[2], sc.keys[2])
        for name in ("buf", "wet", "bus"):
            assert same(out[name], got[name][2]) == ramp, (name, ramp)


@pytest.mark.parametrize("T,B", SHAPES, ids=IDS)
def test_cut_and_resumed_from_copied_state(T, B):
    sc = scenario(T, B)
    got, whole = reference(T, B)
    head = HostStrip(sc)
    first = head.run(0, 3)
    tail = copy.deepcopy(head)
    for twin in (head.eq, head.bus_eq):                                        # the copy shares nothing with its source
        twin.state[:] = np.nan
    head.dyn.s[:] = np.nan
    head.delay.line.hist[:] = np.nan
    head.reverb.hist[:] = np.nan
    head.meter.ring[:] = np.nan
    rest = tail.run(3, N_BUFFERS)
    for name in OUTPUTS:
        assert same(np.concatenate([first[name], rest[name]]), got[name]), name
    assert first["counts"] + rest["counts"] == got["counts"]
    # and the twins end where the uncut strip's ended
    for a, b in ((tail.eq, whole.eq), (tail.bus_eq, whole.bus_eq)):
        assert same(a.state, b.state)
    assert same(tail.dyn.s, whole.dyn.s) and same(tail.delay.line.hist, whole.delay.line.hist)
    assert same(tail.reverb.hist, whole.reverb.hist) and same(tail.reverb.q, whole.reverb.q)
    assert same(tail.resample.hist, whole.resample.hist) and tail.resample.k == whole.resample.k
    assert same(tail.meter.ring, whole.meter.ring) and same(tail.bus_meter.hist, whole.bus_meter.hist)


def test_differing_names_what_differs():
    a = {"x": np.array([1.0, np.nan], np.float32), "counts": [1, 2]}
    b = {"x": np.array([1.0, np.nan], np.float32), "counts": [1, 2]}
    assert differing(a, b) == []
    b["x"] = np.array([1.0, -0.0], np.float32)
    b["counts"] = [1, 3]
    assert differing(a, b) == ["counts", "x"]
    assert not same(np.array([0.0], np.float32), np.array([-0.0], np.float32))
