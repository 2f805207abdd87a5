"""The delay plan (gab_delay_*) on the device.

Every comparison is on bit patterns against delay_reference_f32 (tests/test_delay_host.py) run through a host Twin of the
plan's state machine, unless the test says otherwise: the contract fixes every rounding, so the kernel has no freedom.
The known-answer tests (integer shifts, the echo of an impulse) hold the kernel without trusting that reference.
The reference streams are computed once per (shape, interp, scenario) and shared.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_delay_host import (INTERPS, Twin, capacity, delay_mix, min_delay, noise, table)

pytestmark = pytest.mark.gpu

# (tracks, bufsize, max_delay, buffers).  2 * capacity / B + 2 buffers where the wrap is the point (capacity 256 and 2048),
# three or four where the capacity is large (a steady buffer, the ramp buffer, the steady buffer behind it).
SHAPES = [(5, 100, 37, 8), (64, 64, 1000, 66), (130, 512, 4096, 4), (4100, 512, 600, 3), (3, 2048, 70000, 3), (1, 1, 2, 20)]


def run(plan, x):
    """x [T][B] numpy -> [T][B] numpy"""
    return host(plan.process(dev(x.ravel()))).reshape(plan.tracks, plan.bufsize)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def same_line(plan, line):
    """The ring's newest max_delay + 3 values (as many as the stream has had) are the twin's, and the positions its
    sample count."""
    ring, pos = (host(a) for a in plan.line())
    cap = ring.shape[1]
    assert cap == capacity(plan.bufsize, plan.max_delay)
    if not (pos == line.count % cap).all():
        return False
    H = line.hist.shape[1]
    idx = (line.count - H + np.arange(H)) % cap
    return np.array_equal(bits(ring[:, idx]), bits(line.hist))


@functools.lru_cache(maxsize=None)
def stream(T, B, M, interp, n, ramp_at):
    """The shared scenario: parameters delay_mix(seed 1) at once, delay_mix(seed 2) set with a ramp before buffer ramp_at,
    n buffers of noise.  Returns (p0, p1, xs [n][T][B], ys [n][T][B], the twin afterwards); read only."""
    p0, p1 = delay_mix(T, B, M, interp, 1), delay_mix(T, B, M, interp, 2)
    twin = Twin(T, B, M, interp)
    twin.set_params(p0, ramp=False)
    xs = np.stack([noise(T, B, 1000 + k) for k in range(n)])
    ys = []
    for k in range(n):
        if k == ramp_at:
            twin.set_params(p1)
        ys.append(twin.process(xs[k]))
    ys = np.stack(ys)
    for a in (p0, p1, xs, ys):
        a.setflags(write=False)
    return p0, p1, xs, ys, twin


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("T,B,M,n", SHAPES)
def test_contract_bit_for_bit(gab, T, B, M, n, interp):
    """A steady buffer, a ramp buffer, the tables after the ramp, the steady buffers behind it, the lines at the end."""
    p0, p1, xs, ys, twin = stream(T, B, M, interp, n, 1)
    plan = gab.DelayPlan(T, B, M, interp)
    assert (plan.tracks, plan.bufsize, plan.max_delay, plan.min_delay) == (T, B, M, min_delay(interp))
    plan.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == 1:
            plan.set_params(dev(p1))
            assert same_params(plan, p0, p1)
        assert np.array_equal(bits(run(plan, xs[k])), bits(ys[k])), k
        if k == 1:
            assert same_params(plan, p1, p1)
    assert same_line(plan, twin.line)
    plan.close()


def test_a_new_plan_is_pass_through(gab):
    for interp in INTERPS:
        plan = gab.DelayPlan(7, 50, 90, interp)
        assert same_params(plan, table(7, min_delay(interp), 0, 0, 1), table(7, min_delay(interp), 0, 0, 1))
        x = noise(7, 50, 5)
        assert np.array_equal(bits(run(plan, x)), bits(x))
        plan.close()


# ---- 2. a ramp that crosses the forms within one buffer ---------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("B", [100, 512])
def test_a_ramp_across_the_forms(gab, interp, B):
    """300 to min_delay and back, B + 50 to B - 50 and back, with feedback: within one buffer the chunks go from wider
    than a wave to one sample, and from the ring alone to the buffer's own values."""
    lo, T, M = min_delay(interp), 6, 700
    a = np.array([[300, 0.5, 1, 0.5], [lo, -0.5, 1, 0], [B + 50, 0.6, 0.7, 0.2], [B - 50, -0.6, 1, 1],
                  [300.25, 0.0, 1, 0], [lo + 0.5, 0.7, -1, 0.3]], np.float32)
    b = a[[1, 0, 3, 2, 5, 4]].copy()
    plan, twin = gab.DelayPlan(T, B, M, interp), Twin(T, B, M, interp)
    plan.set_params(dev(a), ramp=False)
    twin.set_params(a, ramp=False)
    for k in range(7):
        if k in (1, 3, 5):
            nxt = b if k != 3 else a
            plan.set_params(dev(nxt))
            twin.set_params(nxt)
        x = noise(T, B, 40 + k)
        assert np.array_equal(bits(run(plan, x)), bits(twin.process(x))), k
    assert same_line(plan, twin.line)
    plan.close()


# ---- 3. known answers: no reference needed ------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("B", [100, 64, 1])
def test_integer_delays_are_exact_shifts(gab, interp, B):
    D = np.array([2, 5, 63, 64, 65, 100, 137, 300, 2, 511], np.int64)
    T, n = len(D), max(8, 1200 // B)
    plan = gab.DelayPlan(T, B, 511, interp)
    plan.set_params(dev(table(T, D.astype(np.float32))), ramp=False)
    x = noise(T, n * B, 7)
    y = np.concatenate([run(plan, x[:, k * B:(k + 1) * B]) for k in range(n)], axis=1)
    for t in range(T):
        assert not y[t, :D[t]].any()
        assert np.array_equal(bits(y[t, D[t]:]), bits(x[t, :n * B - D[t]])), (t, D[t])
    plan.close()


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("batch", [False, True])
def test_known_answer_echo(gab, interp, batch):
    B, n = 64, 16
    D = np.array([2, 3, 7, 24, 64, 100, 333], np.int64)
    T = len(D)
    plan = gab.DelayPlan(T, B, 400, interp)
    plan.set_params(dev(table(T, D.astype(np.float32), fb=0.5)), ramp=False)
    x = np.zeros((n, T, B), np.float32)
    x[0, :, 0] = 1.0
    if batch:
        y = host(plan.process_batch(dev(x.ravel()))).reshape(n, T, B)
    else:
        y = np.stack([run(plan, x[k]) for k in range(n)])
    y = y.transpose(1, 0, 2).reshape(T, n * B)
    for t in range(T):
        want = np.zeros(n * B, np.float32)
        for k in range(1, (n * B - 1) // D[t] + 1):
            want[k * D[t]] = 0.5 ** (k - 1)
        assert np.array_equal(y[t], want), (t, D[t])
    plan.close()


# ---- 4. batches -------------------------------------------------------------------------------------------------
BATCH_SHAPE = (9, 100, 150)          # capacity 256: every batch of 7 or more wraps; every delay class is present


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_batch_is_n_single_launches(gab, n, interp):
    """A ramp is pending at the start.  The batch, n per-buffer calls and the reference agree; so do the two plans'
    rings, positions and tables afterwards."""
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 0)
    a, b = gab.DelayPlan(T, B, M, interp), gab.DelayPlan(T, B, M, interp)
    for p in (a, b):
        p.set_params(dev(p0), ramp=False)
        p.set_params(dev(p1))
    singles = np.stack([run(a, xs[k]) for k in range(n)])
    batch = host(b.process_batch(dev(xs[:n].ravel()))).reshape(n, T, B)
    assert np.array_equal(bits(batch), bits(singles))
    assert np.array_equal(bits(batch), bits(ys[:n]))
    (ra, pa), (rb, pb) = a.line(), b.line()
    assert np.array_equal(bits(host(ra)), bits(host(rb))) and np.array_equal(host(pa), host(pb))
    assert (host(pb) == (n * B) % capacity(B, M)).all()
    assert same_params(a, p1, p1) and same_params(b, p1, p1)
    a.close()
    b.close()


@pytest.mark.parametrize("interp", INTERPS)
def test_a_batch_of_long_buffers(gab, interp):
    """2048-sample buffers are walked in four parts inside the launch; a batch of them equals the single launches."""
    T, B, M, n = 3, 2048, 70000, 3
    p0, p1, xs, ys, twin = stream(T, B, M, interp, n, 1)
    plan = gab.DelayPlan(T, B, M, interp)
    plan.set_params(dev(p0), ramp=False)
    y0 = run(plan, xs[0])
    plan.set_params(dev(p1))
    rest = host(plan.process_batch(dev(xs[1:].ravel()))).reshape(n - 1, T, B)
    assert np.array_equal(bits(y0), bits(ys[0])) and np.array_equal(bits(rest), bits(ys[1:]))
    assert same_line(plan, twin.line)
    plan.close()


# ---- 5. process and process_batch mixed -------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_mixed_calls_are_the_per_buffer_stream(gab, interp):
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 4)
    plan = gab.DelayPlan(T, B, M, interp)
    plan.set_params(dev(p0), ramp=False)
    got, k = [], 0
    for count in (1, 3, 0, 5, 1, 1, 7, 2):           # 0: the ramp is set here, before buffer 4; it runs in a batch
        if count == 0:
            assert k == 4
            plan.set_params(dev(p1))
        elif count == 1:
            got.append(run(plan, xs[k])[None])
        else:
            got.append(host(plan.process_batch(dev(xs[k:k + count].ravel()))).reshape(count, T, B))
        k += count
    got = np.concatenate(got)
    assert np.array_equal(bits(got), bits(ys[:k]))
    plan.close()


# ---- 6. in place, unaligned -------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("T,B,M", [BATCH_SHAPE, (130, 512, 4096)])
def test_in_place_and_unaligned(gab, interp, T, B, M):
    import torch
    n = 4
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33 if (T, B, M) == BATCH_SHAPE else n, 0 if (T, B, M) == BATCH_SHAPE else 1)
    ramp_at = 0 if (T, B, M) == BATCH_SHAPE else 1
    a, b, c = (gab.DelayPlan(T, B, M, interp) for _ in range(3))
    for p in (a, b, c):
        p.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == ramp_at:
            for p in (a, b, c):
                p.set_params(dev(p1))
        buf = dev(xs[k].ravel())
        assert a.process(buf, out=buf) is buf                                   # in place
        assert np.array_equal(bits(host(buf).reshape(T, B)), bits(ys[k])), k
        big = torch.zeros(T * B + 1, device="cuda")
        big[1:] = dev(xs[k].ravel())
        out = torch.full((T * B + 3,), 7.0, device="cuda")
        b.process(big[1:], out=out[1:T * B + 1])                                # both offset by one float
        o = host(out)
        assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all()
        assert np.array_equal(bits(o[1:T * B + 1].reshape(T, B)), bits(ys[k])), k
        c.process(big[1:], out=big[1:])                                         # in place and unaligned
        assert np.array_equal(bits(host(big)[1:].reshape(T, B)), bits(ys[k])), k
    # a batch in place
    d = gab.DelayPlan(T, B, M, interp)
    d.set_params(dev(p0), ramp=False)
    if ramp_at == 0:
        d.set_params(dev(p1))
        buf = dev(xs[:n].ravel())
        d.process_batch(buf, out=buf)
        assert np.array_equal(bits(host(buf).reshape(n, T, B)), bits(ys[:n]))
    for p in (a, b, c, d):
        p.close()


# ---- 7. one track's knobs moved mid-stream ------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_set_params_tracks_mid_stream(gab, interp):
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 0)
    plan, twin = gab.DelayPlan(T, B, M, interp), Twin(T, B, M, interp)
    plan.set_params(dev(p0), ramp=False)
    twin.set_params(p0, ramp=False)
    still = gab.DelayPlan(T, B, M, interp)
    still.set_params(dev(p0), ramp=False)
    moved = np.zeros(T, bool)
    moved[3:7] = True
    for k in range(6):
        if k == 2:
            plan.set_params(dev(p1[3:6]), first_track=3)                        # with a ramp
            twin.set_params(p1[3:6], first_track=3)
            assert same_params(plan, twin.cur, twin.tgt)
        if k == 4:
            plan.set_params(dev(p1[6:7]), ramp=False, first_track=6)            # at once
            twin.set_params(p1[6:7], ramp=False, first_track=6)
            assert same_params(plan, twin.cur, twin.tgt)
        y, ys_still = run(plan, xs[k]), run(still, xs[k])
        assert np.array_equal(bits(y), bits(twin.process(xs[k]))), k
        assert np.array_equal(bits(y[~moved]), bits(ys_still[~moved])), k        # no other track's bits change
        assert same_params(plan, twin.cur, twin.tgt)
    assert (bits(y[moved]) != bits(ys_still[moved])).any()
    plan.close()
    still.close()


# ---- 8. a shard -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_a_shard_is_those_rows_of_the_whole(gab, interp):
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 0)
    lo, hi = 2, 7
    shard = gab.DelayPlan(hi - lo, B, M, interp)
    shard.set_params(dev(p0[lo:hi]), ramp=False)
    shard.set_params(dev(p1[lo:hi]))
    for k in range(5):
        assert np.array_equal(bits(run(shard, xs[k, lo:hi])), bits(ys[k, lo:hi])), k
    shard.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_a_refused_table_changes_nothing(gab, interp):
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 0)
    lo = min_delay(interp)
    plan = gab.DelayPlan(T, B, M, interp)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    below = np.nextafter(np.float32(lo), np.float32(0))
    cases = [(np.nan, (4, 2)), (np.nan, (0, 0)), (np.inf, (8, 3)), (-np.inf, (2, 1)), (np.inf, (5, 0)), (below, (3, 0)),
             (np.float32(lo - 1), (6, 0)), (np.nextafter(np.float32(M), np.float32(1e9)), (7, 0)), (1.0, (1, 1)),
             (-1.0, (8, 1)), (1.5, (0, 1))]
    for value, where in cases:
        bad = delay_mix(T, B, M, interp, 3)
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, 3] = np.nan                                       # the FIRST offender is named
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d" % where in str(e.value), str(e.value)
    bad = delay_mix(4, B, M, interp, 3)
    bad[2, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), first_track=3)
    assert "track 5 field 1" in str(e.value)
    # the edges themselves are admitted: min_delay, max_delay, a feedback just inside 1
    edge = gab.DelayPlan(3, B, M, interp)
    edge.set_params(dev(np.array([[lo, np.nextafter(np.float32(1), np.float32(0)), 1, 0], [M, -0.5, 0, 1],
                                  [lo, 0, 1e30, -1e30]], np.float32)))
    edge.close()
    assert same_params(plan, p0, p1)
    for k in range(2):                                                          # the pending ramp is still pending
        assert np.array_equal(bits(run(plan, xs[k])), bits(ys[k])), k
    plan.close()
    # A refused RAMPED set on a plan with NO ramp pending: none is pending afterwards, current == target == the old
    # rows, and the next buffers are steady buffers of the old rows.
    T, B, M = 5, 64, 16
    q0 = delay_mix(T, B, M, interp, 4)
    plan, twin = gab.DelayPlan(T, B, M, interp), Twin(T, B, M, interp)
    plan.set_params(dev(q0), ramp=False)
    twin.set_params(q0, ramp=False)
    x = noise(T, B, 50)
    assert np.array_equal(bits(run(plan, x)), bits(twin.process(x)))
    bad = delay_mix(T, B, M, interp, 5)
    bad[4, 1] = 1.0
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), ramp=True)
    assert "track 4 field 1" in str(e.value)
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad[3:]), ramp=True, first_track=3)
    assert "track 4 field 1" in str(e.value)
    for k in range(2):
        assert same_params(plan, q0, q0), k
        x = noise(T, B, 51 + k)
        assert np.array_equal(bits(run(plan, x)), bits(twin.process(x))), k
    plan.close()


# ---- 10. reset --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_reset(gab, interp):
    """After a reset with a ramp pending the stream is a new plan's with the same target."""
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, interp, 33, 0)
    plan, fresh = gab.DelayPlan(T, B, M, interp), gab.DelayPlan(T, B, M, interp)
    plan.set_params(dev(p0), ramp=False)
    for k in range(4):
        run(plan, xs[k])
    plan.set_params(dev(p1))
    plan.reset()
    assert same_params(plan, p1, p1)
    ring, pos = plan.line()
    assert not host(ring).any() and not host(pos).any()
    fresh.set_params(dev(p1), ramp=False)
    twin = Twin(T, B, M, interp)
    twin.set_params(p1, ramp=False)
    for k in range(4, 8):
        y = run(plan, xs[k])
        assert np.array_equal(bits(y), bits(run(fresh, xs[k]))), k
        assert np.array_equal(bits(y), bits(twin.process(xs[k]))), k
    plan.close()
    fresh.close()


# ---- 11. bad arguments ------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, M = BATCH_SHAPE
    p0, p1, xs, ys, _ = stream(T, B, M, "linear", 33, 0)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 10, 0), (4, 0, 10, 0), (4, 64, 0, 0), (4, 64, 1, 1), (4, 64, 2 ** 20 + 1, 0), (4, 64, 10, 2)):
        assert lib.gab_delay_create(ctypes.byref(h), *args) == bad and not h.value, args
    for args in ((4, 64, 10, 7), (0, 64, 10, "linear"), (4, 64, 1, "lagrange3")):
        with pytest.raises((gab.GabError, ValueError)):
            gab.DelayPlan(*args)
    plan = gab.DelayPlan(T, B, M, "linear")
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    hp = plan._h
    buf, out, pd = dev(xs[0].ravel()), dev(np.zeros(T * B, np.float32)), dev(p0)
    q, o, pp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, out, pd))
    assert lib.gab_delay_process(hp, None, o, None) == bad and lib.gab_delay_process(hp, q, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_delay_process_batch(hp, q, o, 0, None) == bad and lib.gab_delay_process_batch(hp, q, o, -3, None) == bad
    assert lib.gab_delay_process_batch(hp, None, o, 1, None) == bad
    assert lib.gab_delay_set_params(hp, None, 1, None) == bad and lib.gab_delay_set_params(None, pp, 1, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_delay_set_params_tracks(hp, pp, first, n, 1, None) == bad, (first, n)
    assert lib.gab_delay_params(hp, None, None, None) == bad and lib.gab_delay_line(hp, None, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:7]))
    for k in range(2):
        assert np.array_equal(bits(run(plan, xs[k])), bits(ys[k])), k
    plan.close()
