"""The reverb plan (gab_reverb_*) on the device.

Every comparison is on bit patterns against reverb_reference_f32 (tests/test_reverb_host.py) run through the host Twin
of the plan's state machine, unless it says otherwise: the contract fixes every rounding, so the kernel has no freedom.
The reference streams are computed once per scenario and shared, read only.

The kernel's cut (k_reverb.hip): a wave owns 64 / N tracks and walks chunks of min(64, its smallest delay) samples;
lanes run along time around a serial phase with a lane per (track, line).  The shapes below leave a wave's last group of
tracks partial, take buffers that are no multiple of 4 or of the chunk, wrap the rings several times, make every delay
the minimum, take a buffer of one sample, and span many chunks over a large ring.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_mix_host import fma32  # noqa: F401 (the restatement's fmaf)
from test_reverb_host import (GMAX, DAMP_MAX, Twin, hadamard_sign, identity, make_row, noise, plain_network, reverb_mix,
                              row_floats)

pytestmark = pytest.mark.gpu

# (tracks, bufsize, lines, outs, max_delay, buffers)
SHAPES = [(5, 100, 4, 1, 150, 8), (9, 64, 8, 2, 1000, 20), (3, 512, 16, 2, 4096, 4), (130, 48, 8, 2, 32, 6),
          (1, 1, 4, 1, 33, 80), (70, 2048, 8, 1, 70000, 3)]
A = (5, 100, 4, 1, 150)        # the batch shape: every line word is read again, warm, many times
S = (9, 64, 8, 2, 1000)        # two outputs; 8 tracks to a wave, so track 8 is a wave of its own


def delay_mix(T, N, max_delay, seed):
    """Random delays in [32, max_delay] per line; track 0 all 32, track 1 all max_delay, track 2 a single 32 among long
    lines: the tracks of one wave have different minima."""
    rng = np.random.RandomState(seed)
    d = rng.randint(32, max_delay + 1, (T, N)).astype(np.int32)
    d[0] = 32
    if T > 1:
        d[1] = max_delay
    if T > 2:
        d[2] = rng.randint((32 + max_delay) // 2, max_delay + 1, N)
        d[2, N // 2] = 32
    return d


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def make(gab, shape):
    T, B, N, O, md = shape[:5]
    return gab.ReverbPlan(T, B, lines=N, outs=O, max_delay=md)


def run(plan, x):
    """x [T][B] numpy -> y [T O][B] numpy"""
    return host(plan.process(dev(x.ravel()))).reshape(plan.tracks * plan.outs, plan.bufsize)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def same_state(plan, twin):
    """The newest max_delay words of every line, the positions, q and the delays."""
    ring, pos, q, delays = (host(t) for t in plan.state())
    cap = ring.shape[2]
    if cap != twin.cap or not (pos == twin.pos).all() or not np.array_equal(delays, twin.delays):
        return False
    at = (twin.pos - twin.max_delay + np.arange(twin.max_delay)) & (cap - 1)
    return same(ring[:, :, at], twin.hist) and same(q, twin.q)


@functools.lru_cache(maxsize=None)
def stream(T, B, N, O, md, n, ramp_at):
    """The shared scenario: delay_mix and reverb_mix(seed 1) at once, reverb_mix(seed 2) set with a ramp before buffer
    ramp_at, n buffers.  Returns (delays, p0, p1, xs [n][T][B], ys [n][T O][B], the twin afterwards); read only."""
    d, p0, p1 = delay_mix(T, N, md, 5), reverb_mix(T, N, O, 1), reverb_mix(T, N, O, 2)
    twin = Twin(T, B, N, O, md)
    twin.set_delays(d)
    twin.set_params(p0, ramp=False)
    xs = np.stack([noise(T, B, 1000 + k) for k in range(n)])
    ys = []
    for k in range(n):
        if k == ramp_at:
            twin.set_params(p1)
        ys.append(twin.process(xs[k]))
    ys = np.stack(ys)
    for a in (d, p0, p1, xs, ys, twin.hist, twin.q):
        a.setflags(write=False)
    return d, p0, p1, xs, ys, twin


def start(gab, shape, d, p0, p1=None):
    plan = make(gab, shape)
    plan.set_delays(dev(d))
    plan.set_params(dev(p0), ramp=False)
    if p1 is not None:
        plan.set_params(dev(p1))
    return plan


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,N,O,md,n", SHAPES)
def test_contract_bit_for_bit(gab, T, B, N, O, md, n):
    """A table at once, a second ramped in before a middle buffer, the steady buffers behind it; then the tables and the
    state (lines, positions, q, delays)."""
    mid = n // 2
    d, p0, p1, xs, ys, twin = stream(T, B, N, O, md, n, mid)
    plan = start(gab, (T, B, N, O, md), d, p0)
    assert (plan.tracks, plan.bufsize, plan.lines, plan.outs, plan.row_floats) == (T, B, N, O, row_floats(N, O))
    for k in range(n):
        if k == mid:
            plan.set_params(dev(p1))
            assert same_params(plan, p0, p1)
        assert same(run(plan, xs[k]), ys[k]), k
        if k == mid:
            assert same_params(plan, p1, p1)
    assert same_state(plan, twin)
    plan.close()


def test_a_new_plan_is_pass_through_and_a_reset_starts_from_silence(gab):
    for shape in (A, S):
        T, B, N, O, md = shape
        d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 8 if shape == A else 20, 2)
        plan = make(gab, shape)
        ident = identity(T, N, O)
        assert same_params(plan, ident, ident)
        fresh = Twin(T, B, N, O, md)
        assert same_state(plan, fresh)
        y = run(plan, xs[0])
        assert np.array_equal(bits(y.reshape(T, O, B)), bits(np.repeat(xs[0][:, None, :], O, axis=1)))
        # into the scenario, a ramp pending, then reset: the stream restarts from silence with current == target
        plan.set_delays(dev(d))
        plan.set_params(dev(p0), ramp=False)
        for k in range(2):
            run(plan, xs[k])
        plan.set_params(dev(p1))
        plan.reset()
        assert same_params(plan, p1, p1)
        twin = Twin(T, B, N, O, md)
        twin.set_delays(d)
        twin.set_params(p1, ramp=False)
        assert same_state(plan, twin)
        for k in range(3):
            assert same(run(plan, xs[k]), twin.process(xs[k])), k
        plan.close()


# ---- 2. batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 6, 33])
def test_batch_is_n_single_launches(gab, n):
    """A ramp is pending in front of the batch.  33 buffers of 100 samples over rings of 256 words: every line word is
    stored and read again, warm, a dozen times inside one launch."""
    T, B, N, O, md = A
    d, p0, p1, xs, ys, twin = stream(T, B, N, O, md, 33, 0)
    a, b = start(gab, A, d, p0, p1), start(gab, A, d, p0, p1)
    singles = np.stack([run(a, xs[k]) for k in range(n)])
    batch = host(b.process_batch(dev(xs[:n].ravel()))).reshape(n, T * O, B)
    assert same(batch, singles) and same(batch, ys[:n])
    for p in (a, b):
        assert same_params(p, p1, p1)
    assert all(same(host(u), host(v)) for u, v in zip(a.state(), b.state()))
    if n == 33:
        assert same_state(b, twin)
    else:
        assert same(run(b, xs[n]), ys[n])                             # and the stream goes on
    a.close()
    b.close()


def test_mixed_calls_are_the_per_buffer_stream(gab):
    T, B, N, O, md = S
    d, p0, p1, xs, ys, twin = stream(T, B, N, O, md, 20, 3)
    plan = start(gab, S, d, p0)
    got = [run(plan, xs[0])[None], host(plan.process_batch(dev(xs[1:3].ravel()))).reshape(2, T * O, B)]
    plan.set_params(dev(p1))                                          # the ramp runs through the batch's first buffer
    got.append(host(plan.process_batch(dev(xs[3:12].ravel()))).reshape(9, T * O, B))
    got.append(run(plan, xs[12])[None])
    got.append(host(plan.process_batch(dev(xs[13:20].ravel()))).reshape(7, T * O, B))
    assert same(np.concatenate(got), ys)
    assert same_state(plan, twin)
    plan.close()


# ---- 3. in place, unaligned -------------------------------------------------------------------------------------
def test_in_place_and_unaligned(gab):
    import torch
    T, B, N, O, md = A
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 33, 0)
    a, b, c = (start(gab, A, d, p0, p1) for _ in range(3))
    for k in range(3):
        buf = dev(xs[k].ravel())
        assert a.process(buf, out=buf) is buf                                    # in place: outs == 1
        assert same(host(buf).reshape(T, B), ys[k]), k
        big = torch.zeros(T * B + 1, device="cuda")
        big[1:] = dev(xs[k].ravel())
        out = torch.full((T * B + 3,), 7.0, device="cuda")
        b.process(big[1:], out=out[1:T * B + 1])                                 # in and out offset by one float
        o = host(out)
        assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all()
        assert same(o[1:T * B + 1].reshape(T, B), ys[k]), k
        c.process(big[1:], out=big[1:])                                          # in place and unaligned
        assert same(host(big)[1:].reshape(T, B), ys[k]), k
    for p in (a, b, c):
        p.close()
    # two outputs: unaligned works, in place is refused and changes nothing
    T, B, N, O, md = S
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    plan = start(gab, S, d, p0)
    big = torch.zeros(T * B + 1, device="cuda")
    out = torch.full((T * O * B + 3,), 7.0, device="cuda")
    for k in range(2):
        big[1:] = dev(xs[k].ravel())
        if k == 1:
            both = torch.zeros(T * O * B, device="cuda")
            both[:T * B] = big[1:]
            q = ctypes.c_void_p(both.data_ptr())
            assert gab.lib.gab_reverb_process(plan._h, q, q, None) == gab._capi.GAB_ERR_INVALID_ARG
            assert b"outs == 1" in gab.lib.gab_last_error()
            assert gab.lib.gab_reverb_process_batch(plan._h, q, q, 1, None) == gab._capi.GAB_ERR_INVALID_ARG
        plan.process(big[1:], out=out[1:T * O * B + 1])
        o = host(out)
        assert o[0] == 7.0 and (o[T * O * B + 1:] == 7.0).all()
        assert same(o[1:T * O * B + 1].reshape(T * O, B), ys[k]), k
    plan.close()


# ---- 4. tables moved mid-stream ---------------------------------------------------------------------------------
def test_tables_mid_stream(gab):
    """New delays act from the next buffer and keep the lines; sets on a range that starts inside a wave's group of
    tracks (8 tracks at N = 8: tracks 3..6, and 7..8 across two waves) touch only their rows."""
    T, B, N, O, md = S
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    p2, d2, d3 = reverb_mix(T, N, O, 3), delay_mix(T, N, md, 6), delay_mix(T, N, md, 7)
    plan, still, twin = start(gab, S, d, p0), start(gab, S, d, p0), Twin(T, B, N, O, md)
    twin.set_delays(d)
    twin.set_params(p0, ramp=False)
    moved = np.zeros(T, bool)
    for k in range(10):
        if k == 2:                                                    # every delay moves, the lines stay
            plan.set_delays(dev(d2))
            twin.set_delays(d2)
            still.set_delays(dev(d2))
        if k == 4:                                                    # two sets before a buffer: the ramp starts from current
            for q in (p2[3:7], p1[3:7]):
                plan.set_params(dev(q), first_track=3)
                twin.set_params(q, first_track=3)
            moved[3:7] = True
        if k == 6:
            plan.set_delays(dev(d3[7:9]), first_track=7)
            twin.set_delays(d3[7:9], first_track=7)
            plan.set_params(dev(p2[7:9]), ramp=False, first_track=7)             # at once
            twin.set_params(p2[7:9], ramp=False, first_track=7)
            moved[7:9] = True
        assert same_params(plan, twin.cur, twin.tgt), k
        y, ys_still = run(plan, xs[k]).reshape(T, O, B), run(still, xs[k]).reshape(T, O, B)
        assert same(y.reshape(T * O, B), twin.process(xs[k])), k
        assert same(y[~moved], ys_still[~moved]), k                   # no other track's bits change
        if k in (4, 6):
            assert (bits(y[moved]) != bits(ys_still[moved])).any()
        assert same_params(plan, twin.cur, twin.tgt), k
    assert same_state(plan, twin)
    plan.close()
    still.close()


# ---- 5. a shard -------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, B, N, O, md, n = 30, 48, 8, 2, 300, 4                          # 8 tracks to a wave
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, n, n // 2)
    lo, hi = 1, 22                                                    # no multiple of 8 at either end; other minima per wave
    shard = start(gab, (hi - lo, B, N, O, md), d[lo:hi], p0[lo:hi])
    for k in range(n):
        if k == n // 2:
            shard.set_params(dev(p1[lo:hi]))
        assert same(run(shard, xs[k, lo:hi]), ys[k, lo * O:hi * O]), k
    shard.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def test_refused_sets_change_nothing(gab):
    T, B, N, O, md = S
    P = row_floats(N, O)
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    plan = start(gab, S, d, p0)
    for k in range(3):
        assert same(run(plan, xs[k]), ys[k]), k
    plan.set_params(dev(p1))                                          # the pending ramp of buffer 3
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))     # noqa: E731
    cases = [(up(GMAX[N]), (1, 3)), (-up(GMAX[N]), (0, 0)), (1.0, (2, N + 1)), (np.float32(-1e-30), (3, 2 * N - 1)),
             (up(DAMP_MAX), (0, N)), (np.nan, (4, 2 * N + 3)), (np.inf, (8, 3 * N)), (-np.inf, (3, P - 1)), (np.nan, (0, 5))]
    twin = Twin(T, B, N, O, md)
    for value, where in cases:
        bad = reverb_mix(T, N, O, 3)
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, P - 1] = np.nan                         # the FIRST offender is named
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d " % where in str(e.value), str(e.value)
        with pytest.raises(Exception, match="track %d field %d$" % where):        # the twin's check names the same
            twin.set_params(bad)
    bad = reverb_mix(4, N, O, 3)
    bad[2, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), first_track=3)
    assert "track 5 field 1 " in str(e.value)
    for value, where in ((31, (2, 5)), (md + 1, (0, 1)), (0, (8, 0)), (-7, (3, 7))):
        bad = delay_mix(T, N, md, 8)
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, 0] = 31
        with pytest.raises(gab.GabError) as e:
            plan.set_delays(dev(bad))
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG and "track %d line %d " % where in str(e.value), str(e.value)
    bad = delay_mix(3, N, md, 8)
    bad[1, 4] = md + 1
    with pytest.raises(gab.GabError) as e:
        plan.set_delays(dev(bad), first_track=6)
    assert "track 7 line 4 " in str(e.value)
    # the edges themselves are admitted
    edge = make(gab, (2, B, N, O, md))
    rows = reverb_mix(2, N, O, 4)
    rows[0, :N], rows[1, :N], rows[0, N:2 * N], rows[1, N:2 * N] = GMAX[N], -GMAX[N], DAMP_MAX, 0.0
    edge.set_params(dev(rows))
    edge.set_delays(dev(np.array([[32] * N, [md] * N], np.int32)))
    edge.close()
    # identical to never having called: the tables, the delays, and the pending ramp is still pending
    assert same_params(plan, p0, p1)
    assert np.array_equal(host(plan.state()[3]), d)
    for k in range(3, 6):
        assert same(run(plan, xs[k]), ys[k]), k
    plan.close()


def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, N, O, md = S
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 8, 2, 100), (4, 0, 8, 2, 100), (4, 64, 5, 2, 100), (4, 64, 8, 3, 100), (4, 64, 8, 2, 31)):
        assert lib.gab_reverb_create(ctypes.byref(h), *args) == bad and not h.value, args
    with pytest.raises(gab.GabError):
        gab.ReverbPlan(4, 64, lines=6)
    plan = start(gab, S, d, p0)
    hp = plan._h
    buf, out, pd, dd = dev(xs[0].ravel()), dev(np.zeros(T * O * B, np.float32)), dev(p0), dev(d)
    q, o, pp, dp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, out, pd, dd))
    assert lib.gab_reverb_process(hp, None, o, None) == bad and lib.gab_reverb_process(hp, q, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_reverb_process_batch(hp, q, o, 0, None) == bad and lib.gab_reverb_process_batch(hp, q, o, -3, None) == bad
    assert lib.gab_reverb_set_params(hp, None, 1, None) == bad and lib.gab_reverb_set_params(None, pp, 1, None) == bad
    assert lib.gab_reverb_set_delays(hp, None, None) == bad and lib.gab_reverb_set_delays(None, dp, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_reverb_set_params_tracks(hp, pp, first, n, 1, None) == bad, (first, n)
        assert lib.gab_reverb_set_delays_tracks(hp, dp, first, n, None) == bad, (first, n)
    assert lib.gab_reverb_params(hp, None, None, None) == bad and lib.gab_reverb_state(hp, None, None, None, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:7]))
    with pytest.raises(ValueError):
        plan.set_params(dev(p0[:3]))
    with pytest.raises(ValueError):
        plan.set_delays(dev(d[:3]))
    for k in range(3):
        assert same(run(plan, xs[k]), ys[k]), k
    plan.close()


# ---- 7. samples that are not finite -----------------------------------------------------------------------------
def test_nonfinite_samples_stay_in_their_track(gab):
    T, B, N, O, md = S
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    plan, twin, clean = start(gab, S, d, p0), Twin(T, B, N, O, md), Twin(T, B, N, O, md)
    for t in (twin, clean):
        t.set_delays(d)
        t.set_params(p0, ramp=False)
    hit = np.zeros(T, bool)
    hit[[0, 2]] = True                                                # both have a line of 32 samples
    for k in range(6):
        x = xs[k].copy()
        if k == 1:
            x[0, 10] = np.nan
        if k == 2:
            x[2, 63] = -np.inf
        y, want = run(plan, x), twin.process(x)
        assert same(y, want), k
        y = y.reshape(T, O, B)
        untouched = clean.process(xs[k]).reshape(T, O, B)             # the stream without those two samples
        assert np.isfinite(y[~hit]).all() and same(y[~hit], untouched[~hit]), k
        if k >= 4:                                                    # the shortest line has come round: they stay
            assert not np.isfinite(y[hit]).any()
    ring = host(plan.state()[0])
    assert np.isfinite(ring[~hit]).all() and not np.isfinite(ring[hit]).all()
    plan.reset()                                                      # and until a reset
    twin.reset()
    y = run(plan, xs[6])
    assert np.isfinite(y).all() and same(y, twin.process(xs[6]))
    plan.close()


# ---- 8. a captured graph ----------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_plain_calls(gab):
    """Three replays of one captured launch on a single stream (no parallel branches), no ramp pending."""
    import torch
    T, B, N, O, md = S
    d, p0, p1, xs, ys, _ = stream(T, B, N, O, md, 20, 3)
    plan = start(gab, S, d, p0)
    for k in range(4):                                                # buffer 3 is the ramp buffer, by a plain call
        if k == 3:
            plan.set_params(dev(p1))
        assert same(run(plan, xs[k]), ys[k])
    x, out = torch.zeros(T * B, device="cuda"), torch.zeros(T * O * B, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out)
        before = plan.state()
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the capture recorded a launch without running it: the state is still the one behind buffer 3
    assert all(same(host(u), host(v)) for u, v in zip(plan.state(), before))
    for k in range(4, 7):
        x.copy_(dev(xs[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(T * O, B), ys[k]), k
    del graph
    plan.close()


# ---- 9. a known answer, memory ----------------------------------------------------------------------------------
def test_dyadic_impulses_on_the_device(gab):
    """Without the restatement: g = 1 / 4, c = +-0.5, impulses 3 and -2 against exact arithmetic (every value a dyadic
    rational that float32 holds, test_reverb_host.test_dyadic_impulses_are_exact), in buffers of 75 samples."""
    N, O, B, n = 4, 2, 75, 8
    m = (32, 34, 37, 41)
    c = [[0.5 * hadamard_sign(1 + o, i) for i in range(N)] for o in range(O)]
    x = np.zeros(n * B, np.float32)
    x[0], x[5] = 3.0, -2.0
    want, _ = plain_network([float(v) for v in x], m, 0.25, c, n * B)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    plan = gab.ReverbPlan(1, B, lines=N, outs=O, max_delay=41)
    plan.set_delays(dev(np.array([m], np.int32)))
    plan.set_params(dev(make_row(N, O, g=0.25, b=1.0, c=c)[None, :]), ramp=False)
    y = np.concatenate([run(plan, x[None, k * B:(k + 1) * B]) for k in range(n)], axis=1)
    assert np.array_equal(bits(y), bits(want.astype(np.float32)))
    assert np.count_nonzero(y) > n * B
    plan.close()


def test_the_plan_releases_its_device_memory(gab):
    """Free device memory is back where it started after many create / use / close cycles."""
    import torch
    T, B, N, O, md = 2048, 64, 8, 2, 960                               # 64 MiB of lines per plan
    x = dev(noise(1, T * B, 9).ravel())
    out = torch.empty(T * O * B, device="cuda")
    p = dev(np.tile(make_row(N, O, g=0.3, damp=0.2, b=1.0, c=0.1), (T, 1)))

    def cycle():
        plan = gab.ReverbPlan(T, B, lines=N, outs=O, max_delay=md)
        plan.set_params(p)
        plan.process(x, out=out)
        plan.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (128 << 20), (free0, free1)                # 20 leaked plans would hold more than 1 GiB
