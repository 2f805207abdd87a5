"""The gate plan (gab_gate_*) on the device.

Every comparison is on bit patterns, of the output, of `act` and of both carried states, against gate_reference_f32
(tests/test_gate_host.py) run through a host Twin of the plan's state machine: the contract fixes every rounding, so the
kernel has no freedom.  The reference streams are computed once per (shape, link, scenario) and shared, read only.

The kernel's cut (k_gate.hip): a workgroup of four waves owns 64 tracks, a wave 16 of them, and walks chunks of 64
samples with the next chunk's loads in flight; in its pointwise phases a lane holds 4 consecutive rows, so a link group
of 2 or 4 is reduced inside a lane, one of 8 or 16 across lanes 16 and 32 apart, one of 32 or 64 across the workgroup's
waves through LDS.  The shapes below cross every one of those edges: a short last wave, a last workgroup whose upper
waves own nothing (96 tracks of link 32), sizes below, at and above a chunk, one sample, odd sizes.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_gate_host import (CLOSE, G_CLOSED, G_OPEN, HOLD, IDENTITY, OPEN, REL, Twin, bursts, gate_mix, noise, row,
                            table)

pytestmark = pytest.mark.gpu

TRACKS = [1, 3, 64, 65, 130]
BUFSIZES = [1, 7, 64, 65, 200, 512]
LINKED = [(128, 200, 2), (128, 200, 4), (128, 65, 8), (128, 200, 16), (96, 200, 32), (128, 200, 64)]
BATCH_SHAPE = (70, 100, 2)


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def run(plan, x, key=None, with_act=True):
    """x [T][B] numpy -> (y [T][B], act [T] or None) numpy"""
    import torch
    act = torch.full((plan.tracks,), -7, device="cuda", dtype=torch.int32) if with_act else None
    y = plan.process(dev(x.ravel()), key=None if key is None else dev(key.ravel()), act=act)
    return host(y).reshape(plan.tracks, plan.bufsize), (host(act) if with_act else None)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def same_state(plan, twin):
    g, c = plan.state()
    return same(host(g), twin.g) and np.array_equal(host(c), twin.c)


@functools.lru_cache(maxsize=None)
def stream(T, B, link, n, ramp_at, keyed):
    """The shared scenario: gate_mix(seed 1) at once, gate_mix(seed 2) set with a ramp before buffer ramp_at, n buffers.
    Returns (p0, p1, xs [n][T][B], keys or None, ys, acts [n][T], the carried (g, c) behind every buffer); read only."""
    p0, p1 = gate_mix(T, 1), gate_mix(T, 2)
    twin = Twin(T, B, link)
    twin.set_params(p0, ramp=False)
    xs = np.stack([bursts(T, B, 1000 + k) for k in range(n)])
    keys = np.stack([bursts(T, B, 2000 + k) for k in range(n)]) if keyed else None
    ys, acts, states = [], [], []
    for k in range(n):
        if k == ramp_at:
            twin.set_params(p1)
        y, act = twin.process(xs[k], None if keys is None else keys[k])
        ys.append(y), acts.append(act), states.append((twin.g.copy(), twin.c.copy()))
    ys, acts = np.stack(ys), np.stack(acts)
    for a in (p0, p1, xs, ys, acts) + (() if keys is None else (keys,)):
        a.setflags(write=False)
    return p0, p1, xs, keys, ys, acts, states


def state_is(plan, state):
    g, c = plan.state()
    return same(host(g), state[0]) and np.array_equal(host(c), state[1])


def follow(plan, T, B, link, n, ramp_at, keyed):
    """The plan through the shared scenario by per-buffer calls: output, act, tables and both states at every buffer."""
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, n, ramp_at, keyed)
    plan.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == ramp_at:
            plan.set_params(dev(p1))
            assert same_params(plan, p0, p1)
        y, act = run(plan, xs[k], None if keys is None else keys[k], with_act=k != 2)
        assert same(y, ys[k]), k
        assert act is None or np.array_equal(act, acts[k]), k
        assert state_is(plan, states[k]), k
        if k == ramp_at:
            assert same_params(plan, p1, p1)
    return acts


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("B", BUFSIZES)
@pytest.mark.parametrize("T", TRACKS)
def test_contract_bit_for_bit(gab, T, B):
    """Three consecutive buffers: a steady one, a ramp buffer, a steady one behind it; state crosses calls and chunk
    edges."""
    plan = gab.GatePlan(T, B)
    assert (plan.tracks, plan.bufsize, plan.link) == (T, B, 1)
    acts = follow(plan, T, B, 1, 3, 1, False)
    assert T * B < 1000 or (0 < acts.sum() < acts.size * B)           # the scenario opens and shuts gates
    plan.close()


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("T,B,link", LINKED)
def test_linked_detectors(gab, T, B, link, keyed):
    """Thresholds, glides and holds differ within every group (gate_mix); only the detector is shared."""
    plan = gab.GatePlan(T, B, link)
    follow(plan, T, B, link, 3, 1, keyed)
    plan.close()
    p0, _, xs, keys, ys, acts, _ = stream(T, B, link, 3, 1, keyed)
    if not keyed:                                                     # and linking matters in this scenario
        alone = stream(T, B, 1, 3, 1, False)
        assert not np.array_equal(alone[5], acts)


def test_a_new_plan_is_pass_through(gab):
    for T, B, link in ((7, 50, 1), (128, 64, 64)):
        plan = gab.GatePlan(T, B, link)
        ident = np.tile(IDENTITY, (T, 1))
        assert same_params(plan, ident, ident)
        x = (noise(T, B, 5).astype(np.float64) * np.exp(np.random.RandomState(6).uniform(-80, 80, (T, B)))).astype(np.float32)
        x[0, 3], x[T - 1, B - 1], x[T // 2, 0], x[1, 1] = np.inf, -np.inf, -0.0, np.nan
        g, c = plan.state()
        assert (host(g) == 1.0).all() and (host(c) == -1).all()
        twin = Twin(T, B, link)
        y, act = run(plan, x)
        want, want_act = twin.process(x)
        # open = 0: every sample that is not a zero opens the gate, for itself (hold 0); both gains are 1 either way
        assert same(y, x) and same(want, x) and np.array_equal(act, want_act) and same_state(plan, twin)
        assert (twin.g == 1.0).all() and act.any()
        plan.close()


# ---- 2. a key, in place, unaligned ------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("T,B,link", [BATCH_SHAPE, (130, 512, 2), (65, 65, 1)])
def test_key_in_place_and_unaligned(gab, T, B, link, keyed):
    import torch
    n = 3
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, n, 1, keyed)
    a, b, c = (gab.GatePlan(T, B, link) for _ in range(3))
    for p in (a, b, c):
        p.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == 1:
            for p in (a, b, c):
                p.set_params(dev(p1))
        kd = None if keys is None else dev(keys[k].ravel())
        buf = dev(xs[k].ravel())
        assert a.process(buf, key=kd, out=buf) is buf                            # in place
        assert same(host(buf).reshape(T, B), ys[k]), k
        big = torch.zeros(T * B + 1, device="cuda")
        big[1:] = dev(xs[k].ravel())
        out = torch.full((T * B + 3,), 7.0, device="cuda")
        act = torch.full((T + 2,), -7, device="cuda", dtype=torch.int32)
        b.process(big[1:], key=kd, out=out[1:T * B + 1], act=act[1:T + 1])       # in and out offset by one float
        o = host(out)
        assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all()
        assert same(o[1:T * B + 1].reshape(T, B), ys[k]), k
        assert np.array_equal(host(act), np.concatenate([[-7], acts[k], [-7]])), k
        koff = None
        if keys is not None:
            koff = torch.zeros(T * B + 1, device="cuda")
            koff[1:] = kd
            koff = koff[1:]
        c.process(big[1:], key=koff, out=big[1:])                                # in place, everything unaligned
        assert same(host(big)[1:].reshape(T, B), ys[k]), k
        for p in (a, b, c):
            assert state_is(p, states[k]), k
    for p in (a, b, c):
        p.close()


# ---- 3. batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("ramp_at", [None, 0])
def test_batch_of_three_is_three_single_launches(gab, ramp_at, keyed):
    """Steady, and with a ramp pending in front of the batch.  gate_mix holds of 700 samples outlast the buffers of 100:
    the count crosses buffers inside the launch."""
    import torch
    T, B, link = BATCH_SHAPE
    n = 3
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, 6, ramp_at, keyed)
    assert max(int(s[1].max()) for s in states[:n]) > B               # a hold longer than a buffer is running at an edge
    a, b = gab.GatePlan(T, B, link), gab.GatePlan(T, B, link)
    for p in (a, b):
        p.set_params(dev(p0), ramp=False)
        if ramp_at == 0:
            p.set_params(dev(p1))
    singles = [run(a, xs[k], None if keys is None else keys[k]) for k in range(n)]
    act = torch.full((n * T,), -7, device="cuda", dtype=torch.int32)
    batch = host(b.process_batch(dev(xs[:n].ravel()), key=None if keys is None else dev(keys[:n].ravel()), act=act))
    batch = batch.reshape(n, T, B)
    assert same(batch, np.stack([s[0] for s in singles])) and same(batch, ys[:n])
    assert np.array_equal(host(act).reshape(n, T), np.stack([s[1] for s in singles]))
    assert np.array_equal(host(act).reshape(n, T), acts[:n])
    assert state_is(a, states[n - 1]) and state_is(b, states[n - 1])
    last = p1 if ramp_at == 0 else p0
    assert same_params(a, last, last) and same_params(b, last, last)
    assert same(run(b, xs[n], None if keys is None else keys[n])[0], ys[n])      # and the stream goes on
    a.close()
    b.close()


def test_mixed_calls_are_the_per_buffer_stream(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, 6, 2, False)
    plan = gab.GatePlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    got = [run(plan, xs[0], with_act=False)[0][None], host(plan.process_batch(dev(xs[1:2].ravel()))).reshape(1, T, B)]
    plan.set_params(dev(p1))                                          # the ramp runs through the batch's first buffer
    got.append(host(plan.process_batch(dev(xs[2:5].ravel()))).reshape(3, T, B))
    got.append(run(plan, xs[5], with_act=False)[0][None])
    assert same(np.concatenate(got), ys) and state_is(plan, states[5])
    plan.close()


# ---- 4. parameters moved mid-stream -----------------------------------------------------------------------------
def test_set_params_mid_stream(gab):
    """Two sets before one buffer (the ramp starts from current), a middle range of tracks (the other rows' tables and
    bits untouched), a set at once, a reset in the stream."""
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, _ = stream(T, B, link, 6, 0, False)
    p2 = gate_mix(T, 3)
    plan, twin = gab.GatePlan(T, B, link), Twin(T, B, link)
    still = gab.GatePlan(T, B, link)
    for p in (plan, twin, still):
        p.set_params(dev(p0) if p is not twin else p0, ramp=False)
    moved = np.zeros(T, bool)
    moved[20:40] = True
    for k in range(6):
        if k == 1:
            for q in (p2[20:40], p1[20:40]):
                plan.set_params(dev(q), first_track=20)
                twin.set_params(q, first_track=20)
            cur, tgt = plan.params()
            assert np.array_equal(bits(host(cur)), bits(p0))                     # every row's current, the moved ones too
            assert np.array_equal(bits(host(tgt)[~moved]), bits(p0[~moved]))
            assert np.array_equal(bits(host(tgt)[moved]), bits(p1[moved]))
        if k == 3:
            plan.set_params(dev(p2[30:40]), ramp=False, first_track=30)          # at once
            twin.set_params(p2[30:40], ramp=False, first_track=30)
        if k == 4:
            plan.set_params(dev(p0[20:40]), first_track=20)
            twin.set_params(p0[20:40], first_track=20)
            plan.reset()                                              # drops that ramp, keeps its target
            twin.reset()
            still.reset()
            g, c = plan.state()
            assert same(host(g), twin.tgt[:, G_CLOSED]) and (host(c) == -1).all()
        assert same_params(plan, twin.cur, twin.tgt), k
        (y, act), (ys_still, _) = run(plan, xs[k]), run(still, xs[k])
        want, want_act = twin.process(xs[k])
        assert same(y, want) and np.array_equal(act, want_act), k
        assert same(y[~moved], ys_still[~moved]), k                   # no other track's bits change
        assert same_params(plan, twin.cur, twin.tgt) and same_state(plan, twin), k
        if k in (1, 3):
            assert (bits(y[moved]) != bits(ys_still[moved])).any()
    plan.close()
    still.close()


def test_the_hold_is_the_targets_on_a_ramp_buffer_and_may_drop_below_a_running_count(gab):
    T, B = 3, 40
    plan, twin = gab.GatePlan(T, B), Twin(T, B)
    first = table(T, open=0.5, close=0.25, att=0.5, rel=0.5, hold=100)
    for p, t in ((plan, dev(first)), (twin, first)):
        p.set_params(t, ramp=False)
    x = np.zeros((T, B), np.float32)
    x[:, 2] = 0.9                                                     # opens every gate; the count runs down from 100
    assert same(run(plan, x)[0], twin.process(x)[0]) and (twin.c == 100 - (B - 3)).all()
    second = np.stack([row(open=0.5, close=0.25, att=0.5, rel=0.5, hold=5), row(open=0.5, close=0.25, att=0.5, rel=0.5, hold=300),
                       row(open=0.8, close=0.1, att=0.9, rel=0.1, g_open=2.0, hold=0)])
    quiet = np.zeros((T, B), np.float32)
    quiet[1, 7] = quiet[2, 7] = 0.9                                   # re-arms track 1 with the NEW hold, on the ramp buffer
    plan.set_params(dev(second))
    twin.set_params(second)
    y, act = run(plan, quiet)
    want, want_act = twin.process(quiet)
    assert same(y, want) and np.array_equal(act, want_act) and same_state(plan, twin)
    # track 0: the running count of 63 was above the new hold of 5 and just ran on down: open through the buffer
    # track 2's running count gives way to the target's hold of 0 at its loud sample, on the ramp buffer already
    assert want_act.tolist() == [B, B, 8] and twin.c.tolist() == [63 - B, 300 - (B - 8), -1]
    y, act = run(plan, quiet)                                         # the steady buffer behind it
    want, want_act = twin.process(quiet)
    assert same(y, want) and np.array_equal(act, want_act) and same_state(plan, twin)
    assert want_act.tolist() == [63 - B, B, 1]                        # track 2, hold 0: open for its loud sample alone
    plan.close()


def test_reset_shuts_the_gate_at_the_targets_closed_gain(gab):
    T, B = 66, 64
    p = gate_mix(T, 5)
    plan, twin = gab.GatePlan(T, B, 2), Twin(T, B, 2)
    plan.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    x = bursts(T, B, 8)
    assert same(run(plan, x)[0], twin.process(x)[0]) and (twin.c >= 0).any()
    q = gate_mix(T, 6)
    plan.set_params(dev(q))                                           # pending: reset takes the target's g_closed
    twin.set_params(q)
    plan.reset()
    twin.reset()
    g, c = plan.state()
    assert same(host(g), q[:, G_CLOSED]) and (host(c) == -1).all() and same_params(plan, q, q)
    y, act = run(plan, x)
    want, want_act = twin.process(x)
    assert same(y, want) and np.array_equal(act, want_act) and same_state(plan, twin)
    plan.close()


# ---- 5. a shard -------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, 6, 0, True)
    lo, hi = 6, 70                                                    # a multiple of link that is no multiple of 16
    shard = gab.GatePlan(hi - lo, B, link)
    shard.set_params(dev(p0[lo:hi]), ramp=False)
    shard.set_params(dev(p1[lo:hi]))
    for k in range(3):
        y, act = run(shard, xs[k, lo:hi], keys[k, lo:hi])
        assert same(y, ys[k, lo:hi]) and np.array_equal(act, acts[k, lo:hi]), k
        assert state_is(shard, (states[k][0][lo:hi], states[k][1][lo:hi])), k
    shard.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    from test_gate_host import ATT, CAP, gate_first_refused
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, _ = stream(T, B, link, 6, 0, False)
    plan = gab.GatePlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))     # noqa: E731
    good = gate_mix(T, 3)
    cases = [(np.nan, (4, OPEN)), (up(2.0 ** 64), (0, OPEN)), (np.float32(-1e-30), (9, OPEN)), (np.inf, (3, OPEN)),
             (up(good[69, OPEN]), (69, CLOSE)), (np.float32(-1e-30), (5, CLOSE)), (np.nan, (6, CLOSE)), (up(CAP), (10, ATT)),
             (np.float32(-1e-30), (11, ATT)), (1.0, (12, REL)), (np.nan, (13, REL)), (up(256.0), (14, G_OPEN)),
             (np.float32(-1e-30), (15, G_OPEN)), (np.inf, (16, G_CLOSED)), (np.nan, (17, G_CLOSED)), (2.5, (18, HOLD)),
             (up(2.0 ** 24), (19, HOLD)), (-1.0, (20, HOLD)), (np.nan, (21, HOLD))]
    assert {w[1] for _, w in cases} == set(range(7))                   # every field
    for value, where in cases:
        bad = good.copy()
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, G_OPEN] = np.nan                        # the FIRST offender is named
        assert gate_first_refused(bad) == where[0] * 7 + where[1]     # the host twin of the rule agrees
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d" % where in str(e.value), str(e.value)
    bad = gate_mix(4, 3)
    bad[2, CLOSE] = up(bad[2, OPEN])                                  # close above the open of its own row
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), first_track=3)
    assert "track 5 field 1" in str(e.value)
    # the edges themselves are admitted
    edge = gab.GatePlan(3, B, 1)
    edge.set_params(dev(np.array([[2.0 ** 64, 2.0 ** 64, CAP, CAP, 256, 256, 2.0 ** 24], [0, -0.0, 0, 0, 0, 0, -0.0],
                                  [1, 1, 0, CAP, 0, 256, 1]], np.float32)))
    edge.close()
    assert same_params(plan, p0, p1)
    for k in range(2):                                                # the pending ramp is still pending
        assert same(run(plan, xs[k])[0], ys[k]), k
    plan.close()


# ---- 7. where float32 ends --------------------------------------------------------------------------------------
def test_a_closing_gate_decays_through_the_subnormals(gab):
    """g_closed = 0: the gain is multiplied by rel per sample.  With rel <= 1/2 it passes through the subnormals to 0;
    with rel = 0.9 it comes to rest on a subnormal (0.9 x 4 ulp rounds to 4 ulp).  The device must do the same."""
    T, B, n = 3, 256, 6
    p = np.stack([row(open=0.5, rel=0.5), row(open=0.5, rel=0.3), row(open=0.5, rel=0.9)])
    plan, twin = gab.GatePlan(T, B), Twin(T, B)
    plan.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    x, key = np.ones((T, B), np.float32), np.zeros((T, B), np.float32)
    tiny = np.zeros(T, bool)
    for k in range(n):
        y, act = run(plan, x, key)
        want, want_act = twin.process(x, key)
        assert same(y, want) and not act.any() and same_state(plan, twin), k
        tiny |= ((want > 0) & (want < 2.0 ** -126)).any(axis=1)
    assert tiny.all()                                                 # every track's gain was subnormal on the way
    assert twin.g[0] == 0.0 and twin.g[1] == 0.0 and 0.0 < twin.g[2] < 2.0 ** -140
    plan.close()


def test_signed_zeros(gab):
    T, B = 5, 70
    p = gate_mix(T, 2)
    plan, twin = gab.GatePlan(T, B), Twin(T, B)
    plan.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    x = np.where(np.random.RandomState(4).rand(T, B) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    for key in (None, bursts(T, B, 9)):
        y, act = run(plan, x, key)
        want, want_act = twin.process(x, key)
        assert np.array_equal(bits(y), bits(want)) and np.array_equal(act, want_act) and same_state(plan, twin)
        assert np.array_equal(np.signbit(y), np.signbit(x))           # gains are >= 0: every zero keeps its sign
    assert want_act.any()
    plan.close()


def test_nonfinite_samples_reach_the_output_and_nothing_else(gab):
    T, B, link = 66, 100, 2
    p = gate_mix(T, 1)
    plan, clean, twin = gab.GatePlan(T, B, link), gab.GatePlan(T, B, link), Twin(T, B, link)
    for q in (plan, clean):
        q.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    for k in range(3):
        x, key = bursts(T, B, 60 + k), bursts(T, B, 70 + k)
        dirty = x.copy()
        if k < 2:
            dirty[0, 10], dirty[1, 50], dirty[65, 99], dirty[30, 0] = np.nan, np.inf, -np.inf, np.nan
        if k == 1:
            key[2, 5], key[3, 5], key[40, 64], key[64, 99] = np.nan, np.nan, np.inf, -np.inf
        # with a key (k >= 1) the state is that of the clean run: x reaches y and nothing else
        y, act = run(plan, dirty, key if k else None)
        want, want_act = twin.process(dirty, key if k else None)
        assert same(y, want) and np.array_equal(act, want_act) and same_state(plan, twin), k
        # what is not finite leaves where it entered and nowhere else (an infinity times a gain of 0 leaves as a NaN)
        assert np.array_equal(np.isfinite(y), np.isfinite(dirty)), k
        assert (np.isnan(dirty) <= np.isnan(y)).all(), k
        if k:
            run(clean, x, key)
            g, c = clean.state()
            assert state_is(plan, (host(g), host(c))), k
        else:
            run(clean, np.where(np.isnan(dirty), 0, dirty), None)      # a NaN in the detector reads as silence
            g, c = clean.state()
            assert state_is(plan, (host(g), host(c))), k
        g, _ = plan.state()
        assert np.isfinite(host(g)).all()
    plan.close()
    clean.close()
    # in the key: a NaN is ignored, an infinity opens the gate
    T, B = 2, 30
    plan = gab.GatePlan(T, B)
    plan.set_params(dev(table(T, open=0.5, close=0.5, hold=2)), ramp=False)
    key = np.zeros((T, B), np.float32)
    key[0, 5], key[1, 5] = np.nan, np.inf
    y, act = run(plan, np.ones((T, B), np.float32), key)
    assert act.tolist() == [0, 3] and not y[0].any() and np.flatnonzero(y[1]).tolist() == [5, 6, 7]
    plan.close()


# ---- 8. captured graphs -----------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_plain_calls(gab):
    import torch
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, states = stream(T, B, link, 6, 0, True)
    plan = gab.GatePlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    y0, _ = run(plan, xs[0], keys[0])                                 # the ramp buffer, by a plain call
    assert same(y0, ys[0])
    x, key, out = (torch.zeros(T * B, device="cuda") for _ in range(3))
    act = torch.zeros(T, device="cuda", dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out, key=key, act=act)
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert state_is(plan, states[0])                                  # the capture recorded a launch without running it
    for k in range(1, 4):
        x.copy_(dev(xs[k].ravel()))
        key.copy_(dev(keys[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(T, B), ys[k]) and np.array_equal(host(act), acts[k]), k
        assert state_is(plan, states[k]), k
    del graph
    plan.close()


@pytest.mark.parametrize("captured", [False, True])
def test_gate_then_dynamics_in_place_is_the_composed_restatement(gab, captured):
    """GatePlan, then DynamicsPlan, both in place on one buffer and one stream, no host wait between the two launches."""
    import torch
    from test_dynamics_host import Twin as DynTwin, dyn_mix
    T, B, link = BATCH_SHAPE
    pg, pd = gate_mix(T, 1), dyn_mix(T, 1)
    gate, dyn = gab.GatePlan(T, B, link), gab.DynamicsPlan(T, B, link)
    gtwin, dtwin = Twin(T, B, link), DynTwin(T, B, link)
    gate.set_params(dev(pg), ramp=False)
    dyn.set_params(dev(pd), ramp=False)
    gtwin.set_params(pg, ramp=False)
    dtwin.set_params(pd, ramp=False)
    xs = [bursts(T, B, 500 + k) for k in range(3)]
    want = [dtwin.process(gtwin.process(x)[0])[0] for x in xs]
    buf = torch.zeros(T * B, device="cuda")
    if captured:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            ga, da = gate.prepare(buf, buf), dyn.prepare(buf, buf)
            with torch.cuda.graph(graph, stream=side):
                gate.launch(ga)
                dyn.launch(da)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
    for k, x in enumerate(xs):
        buf.copy_(dev(x.ravel()))
        if captured:
            graph.replay()
        else:
            gate.process(buf, out=buf)
            dyn.process(buf, out=buf)
        torch.cuda.synchronize()
        assert same(host(buf).reshape(T, B), want[k]), k
    assert same_state(gate, gtwin) and same(host(dyn.state()), dtwin.s)
    if captured:
        del graph
    gate.close()
    dyn.close()


# ---- 9. bad arguments, memory -----------------------------------------------------------------------------------
def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, acts, _ = stream(T, B, link, 6, 0, False)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 1), (4, 0, 1), (4, 64, 3), (4, 64, 128), (6, 64, 4)):
        assert lib.gab_gate_create(ctypes.byref(h), *args) == bad and not h.value, args
    with pytest.raises(gab.GabError):
        gab.GatePlan(5, 64, 2)
    plan = gab.GatePlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    hp = plan._h
    buf, out, pd = dev(xs[0].ravel()), dev(np.zeros(T * B, np.float32)), dev(p0)
    q, o, pp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, out, pd))
    assert lib.gab_gate_process(hp, None, None, o, None, None) == bad and lib.gab_gate_process(hp, q, None, None, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_gate_process(hp, q, o, o, None, None) == bad and b"overlap" in lib.gab_last_error()   # key on out
    last = ctypes.c_void_p(out.data_ptr() + 4 * (T * B - 1))                                          # key on out's last word
    assert lib.gab_gate_process(hp, q, last, o, None, None) == bad and b"overlap" in lib.gab_last_error()
    assert lib.gab_gate_process_batch(hp, q, None, o, None, 0, None) == bad
    assert lib.gab_gate_process_batch(hp, q, None, o, None, -3, None) == bad
    assert lib.gab_gate_set_params(hp, None, 1, None) == bad and lib.gab_gate_set_params(None, pp, 1, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_gate_set_params_tracks(hp, pp, first, n, 1, None) == bad, (first, n)
        assert b"outside the plan" in lib.gab_last_error()
    assert lib.gab_gate_params(hp, None, None, None) == bad and lib.gab_gate_state(hp, None, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:6]))
    with pytest.raises(ValueError):
        plan.set_params(dev(p0[:3]))
    for k in range(2):
        assert same(run(plan, xs[k])[0], ys[k]), k
    plan.close()


def test_fifty_plans_leave_free_device_memory_where_it_was(gab):
    import torch
    T, B = 16384, 512                                                 # 0.9 MiB of tables and 128 KiB of state per plan
    x = dev(noise(1, T * B, 9).ravel())
    out = torch.empty_like(x)
    p = dev(np.tile(row(open=0.3, close=0.1, att=0.5, rel=0.9, hold=10), (T, 1)))

    def cycle():
        plan = gab.GatePlan(T, B, 2)
        plan.set_params(p)
        plan.process(x, out=out)
        plan.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), (free0, free1)                  # 50 leaked plans would hold more than 50 MiB
