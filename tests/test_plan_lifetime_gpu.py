"""Plans come and go: the conv, link, keep-warm and FDTD plans through everything that makes, re-makes or gives back a
GPU resource of theirs (gab_plan.hpp's owners), at their smallest shapes.

Every test asserts bits.  "Equal" is bit for bit against a second plan of the same shape, created after the first was
closed and fed the same seeded input: a buffer, event or stream that was given back too early, twice, or not at all
shows in the second plan's bits (or in the run), and so does set-up state that survived where it should have been made
anew.  No test provokes a fault or a failing allocation; those paths belong to tests/test_plan_owners_host.py.
"""
import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)

pytestmark = pytest.mark.gpu


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# family, tracks, bufsize, taps, scheme
FAMILIES = [
    ("fused without tail", 2, 512, 300, None),
    ("fused classic with tail", 3, 512, 600, None),
    ("split", 4, 512, 1025, "split"),
    ("uniform", 2, 64, 100, None),
    ("direct fallback", 3, 48, 20, None),
    ("fdl", 1, 128, 300, "fdl"),
]


def conv_life(gab, orc, T, B, L, scheme, before=3, after=2):
    """create, set_ir, `before` streaming buffers, reset, `after` more, close: every output."""
    plan = gab.ConvPlan(T, B, L, scheme=scheme)
    plan.set_ir(dev(orc.noise(T * L, seed=7)))
    ys = [host(plan.process(dev(orc.noise(T * B, seed=20 + n)), mode=gab.CONV_STREAMING)) for n in range(before)]
    plan.reset()
    ys += [host(plan.process(dev(orc.noise(T * B, seed=40 + n)), mode=gab.CONV_STREAMING)) for n in range(after)]
    plan.close()
    return ys


@pytest.mark.parametrize("family,T,B,L,scheme", FAMILIES, ids=[f[0].replace(" ", "_") for f in FAMILIES])
def test_conv_plan_closed_and_made_again_gives_the_same_bits(gab, orc, family, T, B, L, scheme):
    first = conv_life(gab, orc, T, B, L, scheme)
    second = conv_life(gab, orc, T, B, L, scheme)
    assert len(first) == 5 and all(np.abs(y).max() > 0 for y in first)
    assert same(first, second)
    if family == "direct fallback":
        # its two history buffers change places at every buffer: closed here after an even number of buffers (four),
        # above after an odd one (five) — whichever way round they lie, both go
        even = conv_life(gab, orc, T, B, L, scheme, before=3, after=1)
        assert same(even, first[:4])
        assert same(conv_life(gab, orc, T, B, L, scheme), first)


def test_conv_round_trip_state_is_made_at_the_first_round_trip_and_goes_with_the_plan(gab, orc):
    """A classic plan: one device buffer, then two round trips (the first makes the staging buffers, words, events and the
    upload stream), then close; a sibling that never round-trips holds none of that and is closed too."""
    import torch
    T, B, L = 4, 512, 600
    ir = dev(orc.noise(T * L, seed=3))
    xs = [orc.noise(T * B, seed=60 + n) for n in range(3)]
    for _ in range(2):                                        # twice: what the first pair gave back, the second takes again
        a, b = gab.ConvPlan(T, B, L), gab.ConvPlan(T, B, L)
        assert a.scheme == "classic"
        a.set_ir(ir)
        b.set_ir(ir)
        a.round_trip_check()                                  # (no round trip yet: nothing is pending, nothing is made)
        want = [host(b.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
        got = [host(a.process(dev(xs[0]), mode=gab.CONV_STREAMING))]
        h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
        for x in xs[1:]:
            h_in.copy_(torch.from_numpy(x))
            got.append(a.round_trip(h_in, h_out).numpy().copy())
        a.round_trip_check()
        assert same(got, want)
        a.close()
        b.close()


def test_conv_engine_rings_resized_between_starts_carry_one_history(gab, orc):
    """A split plan: rings of 3, then of 4; the engine on rings of 4 takes five buffers; stopped; rings of 3 again, started
    again (its progress words and counters are the first start's), two more; closed.  The seven outputs are
    gab_conv_process_batch's on a sibling plan."""
    import torch
    T, B, L = 4, 512, 1025
    n = T * B
    ir = dev(orc.noise(T * L, seed=5))
    xs = [orc.noise(n, seed=80 + k) for k in range(7)]
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    want = host(b.process_batch(dev(np.concatenate(xs)), 7)).reshape(7, n)
    cur = torch.cuda.current_stream()
    h_in, h_out = torch.empty(n).pin_memory(), torch.empty(n).pin_memory()
    got = []

    def feed(in_ring, out_ring, R, buffers):                  # one in flight: slot k of this start, the flush rung, wait
        for k, x in enumerate(buffers):
            h_in.copy_(torch.from_numpy(x))
            in_ring[k % R].copy_(h_in, non_blocking=True)
            cur.synchronize()
            a.engine_submit(1, flush=True)
            a.engine_wait(k + 1, timeout=8.0)
            h_out.copy_(out_ring[k % R], non_blocking=True)
            cur.synchronize()
            got.append(h_out.numpy().copy())

    three = a.engine_rings(3)
    assert three[0].shape == (3, n) and three[1].shape == (3, n)
    four = a.engine_rings(4)
    assert four[0].shape == (4, n)
    in_ring, out_ring = a.engine_start(4, stream=torch.cuda.Stream())
    assert in_ring.data_ptr() == four[0].data_ptr() and out_ring.data_ptr() == four[1].data_ptr()      # the same rings, not new ones
    feed(in_ring, out_ring, 4, xs[:5])
    a.engine_stop()
    a.engine_rings(3)
    in_ring, out_ring = a.engine_start(3, stream=torch.cuda.Stream())
    assert in_ring.shape == (3, n)
    feed(in_ring, out_ring, 3, xs[5:])
    a.engine_stop()
    assert not a.engine_running()
    a.close()
    b.close()
    assert same(got, list(want))


def test_link_plan_and_keep_warm_come_and_go_and_leave_the_registry_clean(gab, orc):
    """LinkPlan(64): a round trip, closed; again: the same bits.  KeepWarm(1): kicked and closed, which ends its launch and
    takes it off the list of resident launches — the engine of a 4-track plan then starts (it is refused beside a
    keep-warm launch) and gives gab_conv_process's bits."""
    import torch
    x = orc.noise(64, seed=11)
    outs = []
    for _ in range(2):
        link = gab.LinkPlan(64)
        h_out = torch.full((64,), -7.0).pin_memory()
        link.round_trip(torch.from_numpy(x).pin_memory(), h_out)
        link.check()
        outs.append(h_out.numpy().copy())
        link.close()
    assert np.array_equal(bits(outs[0]), bits(x)) and same(outs[:1], outs[1:])

    warm = gab.KeepWarm(1)
    warm.kick()
    assert warm.running()
    warm.close()

    T, B, L = 4, 512, 1025
    n = T * B
    ir = dev(orc.noise(T * L, seed=5))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    xin = orc.noise(n, seed=12)
    want = host(b.process(dev(xin), mode=gab.CONV_STREAMING))
    in_ring, out_ring = a.engine_start(3, stream=torch.cuda.Stream())
    cur = torch.cuda.current_stream()
    h_in, h_out = torch.from_numpy(xin).pin_memory(), torch.empty(n).pin_memory()
    in_ring[0].copy_(h_in, non_blocking=True)
    cur.synchronize()
    a.engine_submit(1, flush=True)
    a.engine_wait(1, timeout=8.0)
    h_out.copy_(out_ring[0], non_blocking=True)
    cur.synchronize()
    a.engine_stop()
    assert np.array_equal(bits(h_out.numpy()), bits(want))
    a.close()
    b.close()


def fdtd_life(gab, orc):
    """An 8^3 room: buffers of 8, 16 and 8 samples (the strips grow once), per-track cells for 2 tracks and then for 3
    (each set drops the captured graphs and the arrays before it): every output, and the pressure grid at the end."""
    import torch
    n = 8
    plan = gab.FdtdPlan(gab.fdtd_default_params(n))
    outs = []

    def run(T, B, seed):
        x = orc.noise(T * B, seed=seed)
        out = torch.zeros(T * B, device="cuda")
        plan.process(dev(x), out, T, B, 0, B)
        plan.status()
        outs.append(host(out))

    for seed, B in enumerate((8, 16, 8)):
        run(2, B, 100 + seed)
    for T in (2, 3):
        rng = np.random.RandomState(T)
        plan.set_track_positions(rng.randint(1, n - 1, size=(T, 3)).astype(np.int32),
                                 rng.randint(1, n - 1, size=(T, 3)).astype(np.int32))
        run(T, 8, 110 + T)
        run(T, 8, 120 + T)                                    # (24 steps: captured chains, kept beside each other)
    outs.append(host(plan.pressure()).ravel())
    plan.close()
    return outs


def test_fdtd_plan_strips_positions_and_graphs_remade_give_a_fresh_plans_bits(gab, orc):
    first = fdtd_life(gab, orc)
    second = fdtd_life(gab, orc)
    assert len(first) == 8 and all(np.isfinite(y).all() for y in first) and np.abs(first[-1]).max() > 0
    assert same(first, second)


def test_fdtd_slab_plan_is_created_at_rest_and_closed(gab):
    """Planes 0..4 of 8: the plan is handed out only when its fields are zeroed and the device is at rest."""
    from gpuaudiobench_amd import fdtd_slabs
    G = gab.fdtd_default_params(8)
    for _ in range(2):
        slab = fdtd_slabs.FdtdSlab(G, 0, 4)
        assert (slab.z_begin, slab.z_end) == (0, 4)
        assert slab.owns_source == (0 <= G.source_z < 4) and slab.owns_receiver == (0 <= G.receiver_z < 4)
        for which in (fdtd_slabs.SEND_UP_P, fdtd_slabs.RECV_UP_P, fdtd_slabs.RECV_UP_VZ):
            plane = host(slab.halo(which))
            assert plane.size == 64 and not bits(plane).any()
        slab.close()
