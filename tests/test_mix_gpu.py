"""The mix-bus plan (gab_mix_*) on the device.

Every comparison is on bit patterns against mix_reference_f32 (tests/test_mix_host.py) called with what plan.form
reports, unless the test says otherwise: the contract fixes the summation order, so the kernel has no rounding freedom.
The known-answer tests (one-hot routing, small integers) hold the kernel without trusting that reference.
"""
import ctypes

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_mix_host import (EPS, gains, mix_ramp, mix_reference_f32, noise, one_hot_case, small_integer_case,
                           tree_bound)
from test_mix_host import Twin as HostTwin

pytestmark = pytest.mark.gpu

LAYOUTS = ("track", "sample")
SHAPES = [(8192, 512, 16), (128, 512, 2), (5, 100, 3), (1000, 128, 64), (64, 64, 1), (130, 2048, 7), (200, 513, 4),
          (65536, 512, 2)]


def arrange(x, layout):
    """x [T][B] -> the flat device input of that layout."""
    return dev((x if layout == "track" else x.T).ravel())


def run(plan, x, layout="track"):
    """x [T][B] numpy -> [M][B] numpy"""
    return host(plan.process(arrange(x, layout), layout=layout)).reshape(plan.buses, plan.bufsize)


def Twin(plan):
    """The host twin (tests/test_mix_host.py) of this plan's shape, given the form the plan reports."""
    return HostTwin(plan.tracks, plan.bufsize, plan.buses, *plan.form)


def same_gains(plan, twin):
    c, t = plan.gains()
    return np.array_equal(bits(host(c)), bits(twin.cur)) and np.array_equal(bits(host(t)), bits(twin.tgt))


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,B,M", SHAPES)
def test_contract_bit_for_bit(gab, T, B, M, layout):
    """A steady buffer, a ramp buffer, the gains after the ramp, and the steady buffer behind it."""
    plan = gab.MixPlan(T, B, M)
    twin = Twin(plan)
    g0, g1 = gains(T, M, T + M), gains(T, M, T + M + 1)
    plan.set_gains(dev(g0), ramp=False)
    twin.set_gains(g0, ramp=False)
    for k in range(3):
        if k == 1:
            plan.set_gains(dev(g1))
            twin.set_gains(g1)
        x = noise(T, B, 100 * k + T % 97)
        assert np.array_equal(bits(run(plan, x, layout)), bits(twin.process(x))), k
        assert same_gains(plan, twin), k
    c, t = plan.gains()
    assert np.array_equal(bits(host(c)), bits(g1)) and np.array_equal(bits(host(t)), bits(g1))
    plan.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,B,M", [(128, 512, 2), (200, 513, 4), (1000, 128, 64), (8192, 512, 16)])
def test_unaligned_pointers(gab, T, B, M, layout):
    """Input and output through views offset by one float: the general kernel, the same bits."""
    import torch
    plan = gab.MixPlan(T, B, M)
    twin = Twin(plan)
    g0, g1 = gains(T, M, 3), gains(T, M, 4)
    plan.set_gains(dev(g0), ramp=False)
    twin.set_gains(g0, ramp=False)
    plan.set_gains(dev(g1))
    twin.set_gains(g1)
    for k in range(2):
        x = noise(T, B, 40 + k)
        buf = torch.zeros(T * B + 1, device="cuda")
        buf[1:] = arrange(x, layout)
        out = torch.full((M * B + 2,), 7.0, device="cuda")
        plan.process(buf[1:], out=out[1:M * B + 1], layout=layout)
        o = host(out)
        assert o[0] == 7.0 and o[-1] == 7.0
        assert np.array_equal(bits(o[1:-1].reshape(M, B)), bits(twin.process(x))), k
    plan.close()


# ---- 2. the two layouts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,M", [(300, 512, 5), (8192, 512, 16), (77, 100, 33)])
def test_layouts_agree_bit_for_bit(gab, T, B, M):
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g0, g1 = gains(T, M, 5), gains(T, M, 6)
    for p in (a, b):
        p.set_gains(dev(g0), ramp=False)
        p.set_gains(dev(g1))
    for k in range(2):
        x = noise(T, B, 50 + k)
        assert np.array_equal(bits(run(a, x, "track")), bits(run(b, x, "sample"))), k
    a.close()
    b.close()


def test_a_conv_plan_output_goes_straight_in(gab):
    """ConvPlan.process writes sample-major: that buffer into the mix as it is, and transposed on the host into a
    track-major twin."""
    T, B, M = 300, 512, 4
    conv = gab.ConvPlan(T, B, 512)
    conv.set_ir(dev(np.random.RandomState(1).uniform(-0.05, 0.05, T * 512).astype(np.float32)))
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    twin = Twin(a)
    g = gains(T, M, 7)
    for p in (a, b, twin):
        p.set_gains(dev(g) if p is not twin else g)
    for k in range(2):
        y = conv.process(dev(noise(T, B, 60 + k).ravel()))            # [B][T]
        tm = np.ascontiguousarray(host(y).reshape(B, T).T)              # [T][B]
        ya = host(a.process(y, layout="sample")).reshape(M, B)
        yb = run(b, tm, "track")
        assert np.array_equal(bits(ya), bits(yb)), k
        assert np.array_equal(bits(ya), bits(twin.process(tm))), k
    for p in (conv, a, b):
        p.close()


# ---- 3. known answers: no reference needed ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("T,B,M", [(300, 50, 6), (8192, 512, 16), (1000, 128, 64), (2000, 256, 2)])
def test_known_answers(gab, T, B, M, layout):
    plan = gab.MixPlan(T, B, M)
    x, g, route = one_hot_case(T, B, M, 11)
    plan.set_gains(dev(g), ramp=False)
    assert np.array_equal(bits(run(plan, x, layout)), bits(x[route]))
    x, g, want = small_integer_case(T, B, M, 12)
    plan.set_gains(dev(g), ramp=False)
    assert np.array_equal(run(plan, x, layout), want)
    plan.close()


# ---- 4. the form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M", [(512, 2), (512, 16), (100, 64), (2048, 33)])
def test_form_depends_on_bufsize_and_buses_only(gab, B, M):
    forms = []
    for T in (5, 1000, 65536):
        p = gab.MixPlan(T, B, M)
        forms.append(p.form)
        p.close()
    assert forms[0] == forms[1] == forms[2]
    L, G = forms[0]
    assert L >= 1 and G >= 1


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("inside", [True, False])
def test_the_cuts_do_not_move_with_the_track_count(gab, layout, inside):
    """A plan of T tracks whose last T - T1 gain rows are zero gives the bits of a plan of T1 tracks on the first T1
    tracks' samples: a zero gain adds an exact zero to a chain, an all-zero leaf or group an exact zero to a sum."""
    T, B, M = 1500, 256, 3
    big = gab.MixPlan(T, B, M)
    L, G = big.form
    T1 = 2 * L * G + L + 7 if inside else 3 * L * G
    assert T1 < T
    small = gab.MixPlan(T1, B, M)
    assert small.form == (L, G)
    g0, g1 = gains(T, M, 8), gains(T, M, 9)
    g0[T1:] = 0.0
    g1[T1:] = 0.0
    for p, rows in ((big, T), (small, T1)):
        p.set_gains(dev(g0[:rows]), ramp=False)
        p.set_gains(dev(g1[:rows]))
    for k in range(2):
        x = noise(T, B, 70 + k)
        assert np.array_equal(bits(run(big, x, layout)), bits(run(small, x[:T1], layout))), k
    big.close()
    small.close()


# ---- 5. batches -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_batch_is_n_single_launches(gab, n, pending, layout):
    T, B, M = 700, 512, 4
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g0, g1 = gains(T, M, 21), gains(T, M, 22)
    for p in (a, b):
        p.set_gains(dev(g0), ramp=False)
        if pending:
            p.set_gains(dev(g1))
    xs = [noise(T, B, 300 + k) for k in range(n)]
    singles = np.stack([run(a, x, layout) for x in xs])
    flat = np.concatenate([host(arrange(x, layout)) for x in xs])
    batch = host(b.process_batch(dev(flat), layout=layout)).reshape(n, M, B)
    assert np.array_equal(bits(batch), bits(singles))
    for ga, gb in zip(a.gains(), b.gains()):
        assert np.array_equal(bits(host(ga)), bits(host(gb)))
    if pending:
        assert np.array_equal(bits(host(b.gains()[0])), bits(g1))
    a.close()
    b.close()


@pytest.mark.parametrize("offset", [0, 2, 1])
@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_wide_lanes_give_the_same_bits(gab, M, offset):
    """The launch gives a lane four or two samples when the input is 16- or 8-byte aligned, bufsize is a multiple of
    that many and the launch has 512 workgroups or more (here: 48 buffers in one launch); everything else takes one
    sample per lane.  offset (in floats) 0: 16-byte aligned (eight buses: two samples at most), 2: 8-byte aligned, two
    samples, 1: one sample.  All of them: the bits of 48 single launches (one sample per lane: too few workgroups), and
    the ramp buffer and the one behind it against the reference."""
    import torch
    T, B, n = 600, 1024, 48
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    twin = Twin(a)
    g0, g1 = gains(T, M, 23), gains(T, M, 24)
    for p in (a, b):
        p.set_gains(dev(g0), ramp=False)
        p.set_gains(dev(g1))
    twin.set_gains(g0, ramp=False)
    twin.set_gains(g1)
    xs = np.random.RandomState(25).uniform(-1.0, 1.0, (n, T, B)).astype(np.float32)
    buf = torch.zeros(n * T * B + 4, device="cuda")
    view = buf[offset:offset + n * T * B]
    view.copy_(dev(xs.ravel()))
    assert view.data_ptr() % 16 == 4 * offset
    batch = host(b.process_batch(view)).reshape(n, M, B)
    singles = np.stack([run(a, xs[k]) for k in range(n)])
    assert np.array_equal(bits(batch), bits(singles))
    for k in range(2):
        assert np.array_equal(bits(batch[k]), bits(twin.process(xs[k]))), k
    a.close()
    b.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_lanes_on_a_large_plan_through_an_unaligned_pointer(gab, layout):
    """65536 x 512 x 2 has the workgroups for four samples per lane in a single buffer; through a view offset by one
    float it takes one sample per lane.  The same bits, and the reference's."""
    import torch
    T, B, M = 65536, 512, 2
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    twin = Twin(a)
    g = gains(T, M, 26)
    for p in (a, b, twin):
        p.set_gains(dev(g) if p is not twin else g)
    x = noise(T, B, 27)
    buf = torch.zeros(T * B + 1, device="cuda")
    buf[1:] = arrange(x, layout)
    ya = run(a, x, layout)
    yb = host(b.process(buf[1:], layout=layout)).reshape(M, B)
    assert np.array_equal(bits(ya), bits(yb))
    assert np.array_equal(bits(ya), bits(twin.process(x)))
    a.close()
    b.close()


@pytest.mark.parametrize("pending", [False, True])
def test_a_batch_longer_than_one_launch_takes(gab, pending):
    """A launch takes at most 64 buffers (fewer when the partial sums of 64 would pass 32 MiB): 150 buffers are three
    launches, and at 3000 x 512 x 64 (3 MiB of partial sums per buffer) 25 buffers are three launches of 10, 10, 5."""
    for T, B, M, n in ((300, 64, 2, 150), (3000, 512, 64, 25)):
        a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
        g0, g1 = gains(T, M, 28), gains(T, M, 29)
        for p in (a, b):
            p.set_gains(dev(g0), ramp=False)
            if pending:
                p.set_gains(dev(g1))
        xs = np.random.RandomState(30).uniform(-1.0, 1.0, (n, T, B)).astype(np.float32)
        singles = np.stack([run(a, xs[k]) for k in range(n)])
        batch = host(b.process_batch(dev(xs.ravel()))).reshape(n, M, B)
        assert np.array_equal(bits(batch), bits(singles)), (T, B, M)
        for ga, gb in zip(a.gains(), b.gains()):
            assert np.array_equal(bits(host(ga)), bits(host(gb)))
        a.close()
        b.close()


def test_set_gains_infers_the_row_count(gab):
    T, B, M = 50, 64, 3
    a, b = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g = gains(T, M, 31)
    a.set_gains(dev(g[10:25]), ramp=False, first_track=10, n_tracks=15)
    b.set_gains(dev(g[10:25]), ramp=False, first_track=10)
    for ga, gb in zip(a.gains(), b.gains()):
        assert np.array_equal(bits(host(ga)), bits(host(gb)))
    with pytest.raises(ValueError):
        b.set_gains(dev(g[:5]), n_tracks=5)
    with pytest.raises(ValueError):
        b.set_gains(dev(g.ravel()[:7]), first_track=0)
    a.close()
    b.close()


# ---- 6. state changes mid-stream ------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_state_changes_mid_stream(gab, layout):
    T, B, M = 600, 256, 5
    plan = gab.MixPlan(T, B, M)
    twin = Twin(plan)
    g = [gains(T, M, 30 + k) for k in range(6)]
    k = [0]

    def step(n=1):
        for _ in range(n):
            x = noise(T, B, 900 + k[0])
            assert np.array_equal(bits(run(plan, x, layout)), bits(twin.process(x))), k[0]
            assert same_gains(plan, twin), k[0]
            k[0] += 1

    def both(fn):
        fn(plan, dev)
        fn(twin, lambda a: a)

    x = noise(T, B, 899)
    assert not run(plan, x, layout).any()                                   # a new plan is silence
    both(lambda p, d: p.set_gains(d(g[0])))                                 # a ramp up from silence, then steady
    step(3)
    both(lambda p, d: p.set_gains(d(g[1])))                                 # two sets before one buffer: the ramp
    both(lambda p, d: p.set_gains(d(g[2])))                                 # starts from the audible gains
    assert np.array_equal(bits(host(plan.gains()[0])), bits(g[0]))
    step(2)
    both(lambda p, d: p.set_gains(d(g[3]), ramp=False))                     # at once: no ramp buffer
    assert np.array_equal(bits(host(plan.gains()[0])), bits(g[3]))
    step(2)
    plan.set_gains(dev(g[4][100:140]), ramp=True, first_track=100, n_tracks=40)     # rows with a ramp
    twin.set_gains(g[4][100:140], ramp=True, first=100)
    assert same_gains(plan, twin)
    step(2)
    plan.set_gains(dev(g[5][7:300]), ramp=False, first_track=7, n_tracks=293)       # rows at once
    twin.set_gains(g[5][7:300], ramp=False, first=7)
    assert same_gains(plan, twin)
    step(2)
    plan.set_gains(dev(g[1][0:10]), ramp=True, first_track=0, n_tracks=10)          # a ramp pending on some rows,
    twin.set_gains(g[1][0:10], ramp=True, first=0)
    plan.set_gains(dev(g[2][500:600]), ramp=False, first_track=500, n_tracks=100)   # other rows set at once
    twin.set_gains(g[2][500:600], ramp=False, first=500)
    step(2)
    both(lambda p, d: p.set_gains(d(g[0])))                                 # reset with a ramp pending: it is dropped
    plan.reset()
    twin.reset()
    assert same_gains(plan, twin) and np.array_equal(bits(host(plan.gains()[0])), bits(g[0]))
    step(2)
    plan.close()


def test_a_refused_matrix_changes_nothing(gab):
    T, B, M = 300, 128, 4
    plan, twin = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g0, g1 = gains(T, M, 41), gains(T, M, 42)
    for p in (plan, twin):
        p.set_gains(dev(g0), ramp=False)
        p.set_gains(dev(g1))
    for value, where in ((np.nan, (17, 2)), (np.inf, (299, 3)), (-np.inf, (0, 0))):
        bad = gains(T, M, 43)
        bad[where] = value
        bad[min(where[0] + 1, T - 1), 3] = np.nan                      # the FIRST offender is named
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_gains(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d bus %d" % where in str(e.value), str(e.value)
    bad = gains(40, M, 44)
    bad[5, 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_gains(dev(bad), first_track=100, n_tracks=40)
    assert "track 105 bus 1" in str(e.value)
    for k in range(2):
        x = noise(T, B, 45 + k)
        assert np.array_equal(bits(run(plan, x)), bits(run(twin, x))), k
        for ga, gb in zip(plan.gains(), twin.gains()):
            assert np.array_equal(bits(host(ga)), bits(host(gb)))
    plan.close()
    twin.close()
    # A refused RAMPED set on a plan with NO ramp pending: none is pending afterwards, current == target == the old
    # gains, and the next buffer is the steady buffer of the old gains.  Two groups, a ragged leaf.
    T, B, M = 300, 96, 3
    plan, twin = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g0 = gains(T, M, 47)
    for p in (plan, twin):
        p.set_gains(dev(g0), ramp=False)
    bad = gains(T, M, 48)
    bad[299, 2] = np.inf
    with pytest.raises(gab.GabError) as e:
        plan.set_gains(dev(bad), ramp=True)
    assert "track 299 bus 2" in str(e.value)
    with pytest.raises(gab.GabError) as e:
        plan.set_gains(dev(bad[250:]), ramp=True, first_track=250)
    assert "track 299 bus 2" in str(e.value)
    for k in range(2):
        for ga in plan.gains():
            assert np.array_equal(bits(host(ga)), bits(g0)), k
        x = noise(T, B, 49 + k)
        y = run(plan, x)
        assert np.array_equal(bits(y), bits(run(twin, x))), k
        assert np.array_equal(bits(y), bits(mix_reference_f32(x, g0, g0, None, *plan.form))), k
    plan.close()
    twin.close()


def test_no_click(gab):
    """On a constant input of ones, over a ramp buffer and the steady buffer behind it, every bus stays within the
    tree's rounding bound of the straight line from the old sum to the new one, so no step between neighbouring
    samples exceeds |new - old| / B plus twice that bound."""
    T, B, M = 1024, 512, 4
    plan = gab.MixPlan(T, B, M)
    L, _ = plan.form
    g0, g1 = gains(T, M, 51), gains(T, M, 52)
    plan.set_gains(dev(g0), ramp=False)
    ones = np.ones((T, B), np.float32)
    before = run(plan, ones)
    plan.set_gains(dev(g1))
    y = np.concatenate([before[:, -1:], run(plan, ones), run(plan, ones)], axis=1).astype(np.float64)
    old, new = g0.astype(np.float64).sum(0), g1.astype(np.float64).sum(0)
    r = np.concatenate([[0.0], (np.arange(B) + 1.0) / B, np.ones(B)])
    line = old[:, None] + (new - old)[:, None] * r[None, :]
    bound = tree_bound(T, L) * np.maximum(np.abs(g0), np.abs(g1)).astype(np.float64).sum(0)
    assert (np.abs(y - line) <= bound[:, None]).all()
    steps = np.abs(np.diff(y, axis=1))
    assert (steps <= (np.abs(new - old) / B + 2 * bound)[:, None]).all()
    plan.close()


# ---- 7. a channel strip ---------------------------------------------------------------------------------------
def test_a_channel_strip_end_to_end(gab):
    """EqPlan on 1024 tracks, MixPlan to a stereo bus, a two-track EqPlan on the buses: the references composed.
    (The equalisers in their ordered form, which eq_reference_f32 states bit for bit.)"""
    from test_eq_host import eq_bank, eq_reference_f32
    T, B, S = 1024, 512, 4
    ceq, cbus = eq_bank(T, S, 61), eq_bank(2, 2, 62)
    eq, bus_eq, mix = gab.EqPlan(T, B, S), gab.EqPlan(2, B, 2), gab.MixPlan(T, B, 2)
    eq.set_coeffs(dev(ceq))
    bus_eq.set_coeffs(dev(cbus))
    rng = np.random.RandomState(63)
    mix.set_stereo(rng.uniform(-30, 6, T), rng.uniform(-1, 1, T), ramp=False)
    twin = Twin(mix)
    twin.set_gains(host(mix.gains()[1]), ramp=False)
    st, st_bus = np.zeros((T, S, 2), np.float32), np.zeros((2, 2, 2), np.float32)
    for k in range(3):
        if k == 1:
            db, pan = rng.uniform(-30, 6, T), rng.uniform(-1, 1, T)
            mix.set_stereo(db, pan)
            twin.set_gains(gab.MixPlan.stereo_gains(db, pan))
        x = noise(T, B, 64 + k)
        y = bus_eq.process(mix.process(eq.process(dev(x.ravel()), sequential=True)), sequential=True)
        ref = eq_reference_f32(twin.process(eq_reference_f32(x, ceq, st)), cbus, st_bus)
        assert np.array_equal(bits(host(y).reshape(2, B)), bits(ref)), k
    for p in (eq, bus_eq, mix):
        p.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(gab):
    T, B, M = 100, 256, 3
    plan, twin = gab.MixPlan(T, B, M), gab.MixPlan(T, B, M)
    g0 = gains(T, M, 71)
    for p in (plan, twin):
        p.set_gains(dev(g0))
    lib, h, bad = gab.lib, plan._h, gab._capi.GAB_ERR_INVALID_ARG
    x = noise(T, B, 72)
    buf, out, gd = dev(x.ravel()), dev(np.zeros(M * B, np.float32)), dev(g0)
    q, o, gp = (ctypes.c_void_p(t.data_ptr()) for t in (buf, out, gd))
    for layout in (2, -1, 7):
        assert lib.gab_mix_process(h, q, o, layout, None) == bad
        assert b"layout" in lib.gab_last_error()
        assert lib.gab_mix_process_batch(h, q, o, 1, layout, None) == bad
    assert lib.gab_mix_process(h, None, o, 0, None) == bad and lib.gab_mix_process(h, q, None, 0, None) == bad
    assert b"null pointer" in lib.gab_last_error()
    assert lib.gab_mix_process_batch(h, q, o, 0, 0, None) == bad and lib.gab_mix_process_batch(h, q, o, -3, 0, None) == bad
    assert lib.gab_mix_process_batch(h, None, o, 1, 0, None) == bad
    assert lib.gab_mix_set_gains(h, None, 1, None) == bad and lib.gab_mix_set_gains(None, gp, 1, None) == bad
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_mix_set_gains_tracks(h, gp, first, n, 1, None) == bad, (first, n)
    assert lib.gab_mix_gains(h, None, None, None) == bad and lib.gab_mix_form(h, None, None) == bad
    with pytest.raises(KeyError):
        plan.process(buf, layout="bus")
    # the pending ramp is still pending, nothing moved
    for k in range(2):
        x = noise(T, B, 73 + k)
        assert np.array_equal(bits(run(plan, x)), bits(run(twin, x))), k
    for ga, gb in zip(plan.gains(), twin.gains()):
        assert np.array_equal(bits(host(ga)), bits(host(gb)))
    plan.close()
    twin.close()


# ---- 9. worth having ------------------------------------------------------------------------------------------
def test_the_mix_beats_the_library_gemm(gab):
    """8192 x 512 into 16 buses, track-major, steady: the median device time of gab_mix_process is below that of
    torch.matmul on the [16 x 8192] and [8192 x 512] float32 operands — what a user of this package has to do today —
    measured here, alternating.  A floor, not the target (tools/mix_bench.py reports the fraction of the memory rate)."""
    import torch
    T, B, M = 8192, 512, 16
    plan = gab.MixPlan(T, B, M)
    g = gains(T, M, 81)
    plan.set_gains(dev(g), ramp=False)
    x = dev(noise(T, B, 82).ravel())
    y = torch.empty(M * B, dtype=torch.float32, device="cuda")
    gt, x2 = dev(np.ascontiguousarray(g.T)), x.view(T, B)
    z = torch.empty(M, B, dtype=torch.float32, device="cuda")
    args = plan.prepare(x, y)

    def mix():
        plan.launch(args)

    def gemm():
        torch.matmul(gt, x2, out=z)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for _ in range(10):
        mix()
        gemm()
    torch.cuda.synchronize()
    t_mix, t_gemm = [], []
    for _ in range(50):
        t_mix.append(timed(mix))
        t_gemm.append(timed(gemm))
    m_mix, m_gemm = float(np.median(t_mix)), float(np.median(t_gemm))
    err = float(np.abs(host(y).reshape(M, B) - host(z)).max())
    print("8192 x 512 x 16: gab_mix_process %.1f us, torch.matmul %.1f us (x%.2f); largest difference %.3g"
          % (m_mix, m_gemm, m_gemm / m_mix, err))
    plan.close()
    assert err <= 1e-3 * float(np.abs(host(z)).max())          # the same product (the library's order is its own)
    assert m_mix < m_gemm, (m_mix, m_gemm)
