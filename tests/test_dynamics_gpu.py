"""The dynamics plan (gab_dyn_*) on the device.

Every comparison is on bit patterns against dyn_reference_f32 (tests/test_dynamics_host.py) run through a host Twin of
the plan's state machine: the contract fixes every rounding, so the kernel has no freedom.  The reference streams are
computed once per (shape, link, scenario) and shared, read only.

The kernel's cut (k_dynamics.hip): a wave owns 64 tracks and walks chunks of 64 samples; in its pointwise phases a lane
holds 16 consecutive rows, so a link group of up to 16 tracks is reduced inside a lane, one of 32 or 64 across lanes
16 and 32 apart.  The shapes below cross every one of those edges.
"""
import ctypes
import functools

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_dynamics_host import IDENTITY, Twin, dyn_mix, noise, row
from test_mix_host import fma32  # noqa: F401 (the restatement's fmaf)

pytestmark = pytest.mark.gpu

# (tracks, bufsize, link): one wave and several, a short last wave, odd sizes, sizes below, at and above a chunk, one
# sample, groups inside a lane (2, 8), across lanes (64) and across waves' boundaries (264 tracks of link 8: the group
# of tracks 64..71 starts a wave, 256..263 is a last wave of eight tracks)
SHAPES = [(1, 1, 1), (2, 3, 2), (63, 65, 1), (64, 64, 64), (65, 200, 1), (130, 512, 2), (264, 200, 8), (128, 65, 64),
          (64, 3, 8)]


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def run(plan, x, key=None, with_gr=True):
    """x [T][B] numpy -> (y [T][B], gr [T] or None) numpy"""
    import torch
    gr = torch.full((plan.tracks,), 7.0, device="cuda") if with_gr else None
    y = plan.process(dev(x.ravel()), key=None if key is None else dev(key.ravel()), gr=gr)
    return host(y).reshape(plan.tracks, plan.bufsize), (host(gr) if with_gr else None)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def levels(T, B, seed):
    """Noise at a level per track between -50 and +6 dB: below, around and above the thresholds of dyn_mix."""
    scale = np.exp2(np.random.RandomState(seed + 77).uniform(-8.0, 1.0, (T, 1)))
    return (noise(T, B, seed) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stream(T, B, link, n, ramp_at, keyed):
    """The shared scenario: dyn_mix(seed 1) at once, dyn_mix(seed 2) set with a ramp before buffer ramp_at, n buffers.
    Returns (p0, p1, xs [n][T][B], keys or None, ys, grs [n][T], the twin afterwards); read only."""
    p0, p1 = dyn_mix(T, 1), dyn_mix(T, 2)
    twin = Twin(T, B, link)
    twin.set_params(p0, ramp=False)
    xs = np.stack([levels(T, B, 1000 + k) for k in range(n)])
    keys = np.stack([levels(T, B, 2000 + k) for k in range(n)]) if keyed else None
    ys, grs = [], []
    for k in range(n):
        if k == ramp_at:
            twin.set_params(p1)
        y, gr = twin.process(xs[k], None if keys is None else keys[k])
        ys.append(y), grs.append(gr)
    ys, grs = np.stack(ys), np.stack(grs)
    for a in (p0, p1, xs, ys, grs) + (() if keys is None else (keys,)):
        a.setflags(write=False)
    return p0, p1, xs, keys, ys, grs, twin


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("T,B,link", SHAPES)
def test_contract_bit_for_bit(gab, T, B, link, keyed):
    """A steady buffer, a ramp buffer, the tables after the ramp, a steady buffer behind it, the state at the end; with
    and without the gain-reduction meter."""
    n = 3
    p0, p1, xs, keys, ys, grs, twin = stream(T, B, link, n, 1, keyed)
    plan = gab.DynamicsPlan(T, B, link)
    assert (plan.tracks, plan.bufsize, plan.link) == (T, B, link)
    plan.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == 1:
            plan.set_params(dev(p1))
            assert same_params(plan, p0, p1)
        y, gr = run(plan, xs[k], None if keys is None else keys[k], with_gr=k != 2)
        assert same(y, ys[k]), k
        assert gr is None or same(gr, grs[k]), k
        if k == 1:
            assert same_params(plan, p1, p1)
    assert same(host(plan.state()), twin.s)
    assert T * B < 1000 or (grs < 0).any()                            # the scenario compresses
    plan.close()


def test_a_new_plan_is_pass_through(gab):
    for T, B, link in ((7, 50, 1), (128, 64, 64)):
        plan = gab.DynamicsPlan(T, B, link)
        ident = np.tile(IDENTITY, (T, 1))
        assert same_params(plan, ident, ident)
        x = (noise(T, B, 5).astype(np.float64) * np.exp(np.random.RandomState(6).uniform(-80, 80, (T, B)))).astype(np.float32)
        x[0, 3], x[T - 1, B - 1], x[T // 2, 0] = np.inf, -np.inf, -0.0
        y, gr = run(plan, x)
        assert np.array_equal(bits(y), bits(x)) and not gr.any() and not host(plan.state()).any()
        plan.close()


# ---- 2. batches -------------------------------------------------------------------------------------------------
BATCH_SHAPE = (70, 100, 2)


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("n", [1, 6])
def test_batch_is_n_single_launches(gab, n, keyed):
    """A ramp is pending in front of the batch and the state is carried over six buffers.  The batch, n per-buffer calls
    and the reference agree; so do the two plans' states and tables afterwards."""
    import torch
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, keyed)
    a, b = gab.DynamicsPlan(T, B, link), gab.DynamicsPlan(T, B, link)
    for p in (a, b):
        p.set_params(dev(p0), ramp=False)
        p.set_params(dev(p1))
    singles = [run(a, xs[k], None if keys is None else keys[k]) for k in range(n)]
    gr = torch.full((n * T,), 7.0, device="cuda")
    batch = host(b.process_batch(dev(xs[:n].ravel()), key=None if keys is None else dev(keys[:n].ravel()), gr=gr))
    batch = batch.reshape(n, T, B)
    assert same(batch, np.stack([s[0] for s in singles])) and same(batch, ys[:n])
    assert same(host(gr).reshape(n, T), np.stack([s[1] for s in singles])) and same(host(gr).reshape(n, T), grs[:n])
    assert same(host(a.state()), host(b.state()))
    assert same_params(a, p1, p1) and same_params(b, p1, p1)
    # and the stream goes on from either
    if n < 6:
        assert same(run(b, xs[n], None if keys is None else keys[n])[0], ys[n])
    a.close()
    b.close()


def test_mixed_calls_are_the_per_buffer_stream(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 2, False)
    plan = gab.DynamicsPlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    got = [run(plan, xs[0], with_gr=False)[0][None], host(plan.process_batch(dev(xs[1:2].ravel()))).reshape(1, T, B)]
    plan.set_params(dev(p1))                                          # the ramp runs through the batch's first buffer
    got.append(host(plan.process_batch(dev(xs[2:5].ravel()))).reshape(3, T, B))
    got.append(run(plan, xs[5], with_gr=False)[0][None])
    assert same(np.concatenate(got), ys)
    plan.close()


# ---- 3. in place, unaligned -------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("T,B,link", [BATCH_SHAPE, (130, 512, 2)])
def test_in_place_and_unaligned(gab, T, B, link, keyed):
    import torch
    n = 2
    ramp_at = 0 if (T, B, link) == BATCH_SHAPE else 1
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6 if (T, B, link) == BATCH_SHAPE else 3, ramp_at, keyed)
    a, b, c = (gab.DynamicsPlan(T, B, link) for _ in range(3))
    for p in (a, b, c):
        p.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == ramp_at:
            for p in (a, b, c):
                p.set_params(dev(p1))
        kd = None if keys is None else dev(keys[k].ravel())
        buf = dev(xs[k].ravel())
        assert a.process(buf, key=kd, out=buf) is buf                            # in place
        assert same(host(buf).reshape(T, B), ys[k]), k
        big = torch.zeros(T * B + 1, device="cuda")
        big[1:] = dev(xs[k].ravel())
        out = torch.full((T * B + 3,), 7.0, device="cuda")
        b.process(big[1:], key=kd, out=out[1:T * B + 1])                         # in and out offset by one float
        o = host(out)
        assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all()
        assert same(o[1:T * B + 1].reshape(T, B), ys[k]), k
        koff = None
        if keys is not None:
            koff = torch.zeros(T * B + 1, device="cuda")
            koff[1:] = kd
            koff = koff[1:]
        c.process(big[1:], key=koff, out=big[1:])                                # in place, everything unaligned
        assert same(host(big)[1:].reshape(T, B), ys[k]), k
    for p in (a, b, c):
        p.close()


# ---- 4. parameters moved mid-stream -----------------------------------------------------------------------------
def test_set_params_mid_stream(gab):
    """Ramp 1 and 0, two sets before one buffer, a middle range of tracks, a reset in the stream."""
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, False)
    p2 = dyn_mix(T, 3)
    plan, twin = gab.DynamicsPlan(T, B, link), Twin(T, B, link)
    still = gab.DynamicsPlan(T, B, link)
    for p in (plan, twin, still):
        p.set_params(dev(p0) if p is not twin else p0, ramp=False)
    moved = np.zeros(T, bool)
    moved[20:40] = True
    for k in range(6):
        if k == 1:                                                    # two sets before a buffer: the ramp starts from current
            for q in (p2[20:40], p1[20:40]):
                plan.set_params(dev(q), first_track=20)
                twin.set_params(q, first_track=20)
        if k == 3:
            plan.set_params(dev(p2[30:40]), ramp=False, first_track=30)         # at once
            twin.set_params(p2[30:40], ramp=False, first_track=30)
        if k == 4:
            plan.set_params(dev(p0[20:40]), first_track=20)
            twin.set_params(p0[20:40], first_track=20)
            plan.reset()                                              # drops that ramp, keeps its target
            twin.reset()
            still.reset()
            assert not host(plan.state()).any()
        assert same_params(plan, twin.cur, twin.tgt), k
        (y, gr), (ys_still, _) = run(plan, xs[k]), run(still, xs[k])
        want, want_gr = twin.process(xs[k])
        assert same(y, want) and same(gr, want_gr), k
        assert same(y[~moved], ys_still[~moved]), k                   # no other track's bits change
        assert same_params(plan, twin.cur, twin.tgt), k
        if k in (1, 3):
            assert (bits(y[moved]) != bits(ys_still[moved])).any()
    plan.close()
    still.close()


# ---- 5. a shard -------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, True)
    lo, hi = 6, 70                                                    # a multiple of link that is no multiple of 16
    shard = gab.DynamicsPlan(hi - lo, B, link)
    shard.set_params(dev(p0[lo:hi]), ramp=False)
    shard.set_params(dev(p1[lo:hi]))
    for k in range(3):
        y, gr = run(shard, xs[k, lo:hi], keys[k, lo:hi])
        assert same(y, ys[k, lo:hi]) and same(gr, grs[k, lo:hi]), k
    shard.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, False)
    plan = gab.DynamicsPlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))     # noqa: E731
    down = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    cap = np.float32(1.0 - 2.0 ** -20)
    cases = [(np.nan, (4, 0)), (up(128.0), (0, 0)), (down(-128.0), (9, 0)), (np.float32(1e-30), (3, 1)), (down(-1.0), (69, 1)),
             (np.float32(-1e-30), (5, 2)), (up(64.0), (6, 2)), (np.inf, (7, 3)), (np.float32(-1e-30), (8, 3)), (up(cap), (10, 4)),
             (np.float32(-1e-30), (11, 4)), (1.0, (12, 5)), (np.nan, (13, 5)), (np.inf, (14, 6)), (np.nan, (15, 6)),
             (np.float32(1e-30), (16, 7)), (-np.inf, (17, 7))]
    assert {w[1] for _, w in cases} == set(range(8))                   # every field
    for value, where in cases:
        bad = dyn_mix(T, 3)
        bad[where] = value
        if where[0] + 1 < T:
            bad[where[0] + 1, 6] = np.nan                             # the FIRST offender is named
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d" % where in str(e.value), str(e.value)
    bad = dyn_mix(4, 3)
    bad[2, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(bad), first_track=3)
    assert "track 5 field 1" in str(e.value)
    # the edges themselves are admitted
    edge = gab.DynamicsPlan(3, B, 1)
    edge.set_params(dev(np.array([[128, -1, 64, 0, cap, 0, -1e30, 0], [-128, 0, 0, 1e30, 0, cap, 1e30, -1e30],
                                  [0, -0.0, 0, 0, 0, 0, 0, -0.0]], np.float32)))
    edge.close()
    assert same_params(plan, p0, p1)
    for k in range(2):                                                # the pending ramp is still pending
        assert same(run(plan, xs[k])[0], ys[k]), k
    plan.close()


# ---- 7. samples that are not finite -----------------------------------------------------------------------------
def test_nonfinite_samples_reach_the_output_and_nothing_else(gab):
    T, B, link = 66, 100, 2
    p = dyn_mix(T, 1)
    p[:, 6] = np.abs(p[:, 6])
    plan, twin = gab.DynamicsPlan(T, B, link), Twin(T, B, link)
    plan.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    for k in range(3):
        x, key = levels(T, B, 60 + k), levels(T, B, 70 + k)
        if k < 2:
            x[0, 10], x[1, 50], x[65, 99], x[30, 0] = np.nan, np.inf, -np.inf, np.nan
        if k == 1:
            key[2, 5], key[3, 5], key[40, 64], key[64, 99] = np.nan, np.nan, np.inf, -np.inf
        y, gr = run(plan, x, key if k else None)
        want, want_gr = twin.process(x, key if k else None)
        assert same(y, want) and same(gr, want_gr), k
        assert np.array_equal(np.isnan(y), np.isnan(x)), k            # a NaN leaves where it entered, an infinity too
        assert np.array_equal(np.isinf(y), np.isinf(x)), k
        s = host(plan.state())
        assert np.isfinite(s).all() and np.isfinite(gr).all() and same(s, twin.s), k
    plan.close()


# ---- 8. a captured graph ----------------------------------------------------------------------------------------
def test_graph_replay_gives_the_bits_of_plain_calls(gab):
    import torch
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, True)
    plan = gab.DynamicsPlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    y0, _ = run(plan, xs[0], keys[0])                                 # the ramp buffer, by a plain call
    assert same(y0, ys[0])
    x, key, out, gr = (torch.zeros(T * B, device="cuda"), torch.zeros(T * B, device="cuda"),
                       torch.zeros(T * B, device="cuda"), torch.zeros(T, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        args = plan.prepare(x, out, key=key, gr=gr)
        state = plan.state()
        with torch.cuda.graph(graph, stream=side):
            plan.launch(args)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the capture recorded a launch without running it: the state is still the one behind buffer 0
    assert same(host(plan.state()), host(state))
    for k in range(1, 4):
        x.copy_(dev(xs[k].ravel()))
        key.copy_(dev(keys[k].ravel()))
        graph.replay()
        torch.cuda.synchronize()
        assert same(host(out).reshape(T, B), ys[k]) and same(host(gr), grs[k]), k
    del graph
    plan.close()


# ---- 9. bad arguments, memory -----------------------------------------------------------------------------------
def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, link = BATCH_SHAPE
    p0, p1, xs, keys, ys, grs, _ = stream(T, B, link, 6, 0, False)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 64, 1), (4, 0, 1), (4, 64, 3), (4, 64, 128), (6, 64, 4)):
        assert lib.gab_dyn_create(ctypes.byref(h), *args) == bad and not h.value, args
    with pytest.raises(gab.GabError):
        gab.DynamicsPlan(5, 64, 2)
    plan = gab.DynamicsPlan(T, B, link)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    hp = plan._h
    buf, out, pd = dev(xs[0].ravel()), dev(np.zeros(T * B, np.float32)), dev(p0)
    q, o, pp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, out, pd))
    assert lib.gab_dyn_process(hp, None, None, o, None, None) == bad and lib.gab_dyn_process(hp, q, None, None, None, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_dyn_process(hp, q, o, o, None, None) == bad and b"overlap" in lib.gab_last_error()   # key on out
    assert lib.gab_dyn_process_batch(hp, q, None, o, None, 0, None) == bad
    assert lib.gab_dyn_process_batch(hp, q, None, o, None, -3, None) == bad
    assert lib.gab_dyn_set_params(hp, None, 1, None) == bad and lib.gab_dyn_set_params(None, pp, 1, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_dyn_set_params_tracks(hp, pp, first, n, 1, None) == bad, (first, n)
    assert lib.gab_dyn_params(hp, None, None, None) == bad and lib.gab_dyn_state(hp, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:7]))
    with pytest.raises(ValueError):
        plan.set_params(dev(p0[:3]))
    for k in range(2):
        assert same(run(plan, xs[k])[0], ys[k]), k
    plan.close()


def test_the_plan_releases_its_device_memory(gab):
    """Free device memory is back where it started after many create / use / close cycles."""
    import torch
    T, B = 16384, 512                                                 # 1 MiB of tables and 64 KiB of state per plan
    x = dev(noise(1, T * B, 9).ravel())
    out = torch.empty_like(x)
    p = dev(np.tile(row(thr=-3.0, slope=-0.5, knee=1.0, att=0.5, rel=0.9), (T, 1)))

    def cycle():
        plan = gab.DynamicsPlan(T, B, 2)
        plan.set_params(p)
        plan.process(x, out=out)
        plan.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), (free0, free1)                  # 40 leaked plans would hold more than 40 MiB
