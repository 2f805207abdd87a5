"""The equaliser plan (gab_eq_*) on the device.

Ordered form (eq_sequential_kernel): bit for bit against eq_reference_f32 (tests/test_eq_host.py).
Scan form (eq_scan_kernel): against float64 (scipy's sosfilt on the float32 coefficients), outputs and final state,
within max(1e-5, 4 e32) of the float64 peak per case, where e32 is what eq_reference_f32 itself loses against float64
on the same inputs (computed here on the CPU; at 16 384 tracks on the first 64).  1e-5 of peak is the project's rule for
re-associated float32 paths (test_iir_wave_scan_with_carried_state); the factor 4 allows for the rounding of the table
and of six combine steps on top of a recursion whose own round-off may already exceed 1e-5.  The state is held to the
same rule with its own e32 and its own peak.  Every case prints its figures and err / e32 (pytest -s).
"""
import ctypes

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_eq_host import (N_BUFFERS, SCAN_CASES, bank_round_off, case_seed, eq_bank, eq_reference_f32, noise)

pytestmark = pytest.mark.gpu


def make_plan(gab, T, B, S, coeffs=None):
    plan = gab.EqPlan(T, B, S)
    if coeffs is not None:
        plan.set_coeffs(dev(coeffs))
    return plan


def run(plan, x, **kw):
    """x [T][B] numpy -> [T][B] numpy"""
    return host(plan.process(dev(x.ravel()), **kw)).reshape(x.shape)


def tolerance(e32):
    return max(1e-5, 4.0 * e32)


# ---- 1. the ordered form, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,S", [(128, 512, 1), (128, 512, 8), (5, 100, 3), (200, 513, 4), (64, 64, 16)])
def test_ordered_form_bit_for_bit(gab, T, B, S):
    coeffs = eq_bank(T, S, case_seed(T, B, S))
    plan = make_plan(gab, T, B, S, coeffs)
    st = np.zeros((T, S, 2), np.float32)
    for k in range(3):
        x = noise(T, B, 70 + k)
        y = run(plan, x, sequential=True)
        ref = eq_reference_f32(x, coeffs, st)
        assert np.array_equal(bits(y), bits(ref)), k
        assert np.array_equal(bits(host(plan.state())), bits(st)), k
    plan.close()


def test_one_section_is_gab_iir_sequential(gab, orc):
    T, B = 128, 512
    c = orc.iir_coeffs(0.25)
    plan = make_plan(gab, T, B, 1, np.broadcast_to(c, (T, 1, 5)).copy())
    st = dev(np.zeros(2 * T, np.float32))
    for k in range(3):
        x = noise(T, B, 80 + k)
        y = run(plan, x, sequential=True)
        ref = host(gab.iir(dev(x.ravel()), c, st, T, B, sequential=True)).reshape(T, B)
        assert np.array_equal(bits(y), bits(ref))
        assert np.array_equal(bits(host(plan.state()).ravel()), bits(host(st)))
    plan.close()


def test_shapes_without_a_scan_take_the_ordered_kernel(gab):
    """process() on a buffer size the scan does not cover, and on unaligned pointers: the sequential kernel's bits."""
    import torch
    T, B, S = 5, 100, 3
    coeffs = eq_bank(T, S, 4)
    plan = make_plan(gab, T, B, S, coeffs)
    assert plan.form == (0, 0)
    st = np.zeros((T, S, 2), np.float32)
    x = noise(T, B, 1)
    assert np.array_equal(bits(run(plan, x)), bits(eq_reference_f32(x, coeffs, st)))
    plan.close()
    T, B = 6, 128
    coeffs = eq_bank(T, S, 5)
    plan = make_plan(gab, T, B, S, coeffs)
    assert plan.form == (2, 1)
    x = noise(T, B, 2)
    buf = torch.zeros(T * B + 1, device="cuda")
    buf[1:] = dev(x.ravel())
    out = torch.empty(T * B + 1, device="cuda")
    plan.process(buf[1:], out=out[1:])
    st = np.zeros((T, S, 2), np.float32)
    assert np.array_equal(bits(host(out[1:]).reshape(T, B)), bits(eq_reference_f32(x, coeffs, st)))
    plan.close()


# ---- 2. the scan form against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,S", SCAN_CASES)
def test_scan_form_against_float64(gab, T, B, S):
    seed = case_seed(T, B, S)
    coeffs = eq_bank(T, S, seed)
    sample = slice(0, 64) if T > 1000 else None
    e_out, e_state, ys, st64 = bank_round_off(T, B, S, seed, coeffs=coeffs, tracks=sample)
    assert e_out <= 1e-4, "the bank tests DF-II round-off, not the kernel: %g" % e_out
    if sample is not None:                   # the reference itself on every track (its float32 twin is not needed there)
        _, _, ys, st64 = bank_round_off(T, B, S, seed, coeffs=coeffs)
    plan = make_plan(gab, T, B, S, coeffs)
    assert plan.form != (0, 0)
    err = peak = 0.0
    for k in range(N_BUFFERS):
        y = run(plan, noise(T, B, 1000 * seed + k))
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    err /= peak
    err_state = float(np.abs(host(plan.state()) - st64).max() / np.abs(st64).max())
    print("eq scan T=%d B=%d S=%d form=%s: outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (T, B, S, plan.form, err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    plan.close()
    assert err <= tolerance(e_out), (err, e_out)
    assert err_state <= tolerance(e_state), (err_state, e_state)


# ---- 3. launch forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_batch_is_n_single_launches(gab, n):
    T, B, S = 128, 512, 4
    coeffs = eq_bank(T, S, 21)
    a, b = make_plan(gab, T, B, S, coeffs), make_plan(gab, T, B, S, coeffs)
    xs = np.stack([noise(T, B, 300 + k) for k in range(n)])
    # both plans mid-stream
    a.process(dev(xs[0].ravel()))
    b.process(dev(xs[0].ravel()))
    singles = np.stack([run(a, xs[k]) for k in range(n)])
    batch = host(b.process_batch(dev(xs.ravel()))).reshape(n, T, B)
    assert np.array_equal(bits(batch), bits(singles))
    assert np.array_equal(bits(host(a.state())), bits(host(b.state())))
    a.close()
    b.close()


@pytest.mark.parametrize("sequential", [False, True])
def test_in_place_is_out_of_place(gab, sequential):
    T, B, S = 130, 256, 8
    coeffs = eq_bank(T, S, 22)
    a, b = make_plan(gab, T, B, S, coeffs), make_plan(gab, T, B, S, coeffs)
    for k in range(3):
        x = noise(T, B, 400 + k)
        ya = run(a, x, sequential=sequential)
        buf = dev(x.ravel())
        b.process(buf, out=buf, sequential=sequential)
        assert np.array_equal(bits(ya.ravel()), bits(host(buf)))
    assert np.array_equal(bits(host(a.state())), bits(host(b.state())))
    a.close()
    b.close()


def test_a_channel_shard_is_the_unsharded_job(gab):
    T, B, S = 1000, 128, 4
    coeffs = eq_bank(T, S, 23)
    whole, shard = make_plan(gab, T, B, S, coeffs), make_plan(gab, 64, B, S, coeffs[192:256])
    assert whole.form == shard.form
    for k in range(3):
        x = noise(T, B, 500 + k)
        assert np.array_equal(bits(run(whole, x)[192:256]), bits(run(shard, x[192:256])))
    assert np.array_equal(bits(host(whole.state())[192:256]), bits(host(shard.state())))
    whole.close()
    shard.close()


# ---- 4. state changes -----------------------------------------------------------------------------------------
def test_set_coeffs_mid_stream_ordered_form(gab):
    T, B, S = 40, 256, 4
    c1, c2 = eq_bank(T, S, 31), eq_bank(T, S, 32)
    plan = make_plan(gab, T, B, S, c1)
    st = np.zeros((T, S, 2), np.float32)
    for k in range(6):
        if k == 3:
            plan.set_coeffs(dev(c2))
        x = noise(T, B, 600 + k)
        assert np.array_equal(bits(run(plan, x, sequential=True)), bits(eq_reference_f32(x, c1 if k < 3 else c2, st))), k
    assert np.array_equal(bits(host(plan.state())), bits(st))
    plan.close()


def test_set_coeffs_mid_stream_scan_form(gab):
    T, B, S, seed = 40, 256, 4, 33
    c1, c2 = eq_bank(T, S, 31), eq_bank(T, S, 32)
    e_out, e_state, ys, st64 = bank_round_off(T, B, S, seed, coeffs=c1, n_buffers=6, switch=(3, c2))
    plan = make_plan(gab, T, B, S, c1)
    err = peak = 0.0
    for k in range(6):
        if k == 3:
            plan.set_coeffs(dev(c2))
        y = run(plan, noise(T, B, 1000 * seed + k))
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    err_state = float(np.abs(host(plan.state()) - st64).max() / np.abs(st64).max())
    print("eq scan, coefficients switched at buffer 3: outputs %.3g of peak (e32 %.3g), state %.3g (e32 %.3g)"
          % (err / peak, e_out, err_state, e_state))
    plan.close()
    assert err / peak <= tolerance(e_out) and err_state <= tolerance(e_state)


@pytest.mark.parametrize("sequential", [False, True])
def test_set_coeffs_tracks_leaves_the_other_tracks_alone(gab, sequential):
    T, B, S = 20, 512, 8
    c1, c2 = eq_bank(T, S, 34), eq_bank(T, S, 35)
    plan, twin = make_plan(gab, T, B, S, c1), make_plan(gab, T, B, S, c1)
    mixed = c1.copy()
    mixed[5:9] = c2[5:9]
    st = np.zeros((T, S, 2), np.float32)
    others = np.r_[0:5, 9:T]
    for k in range(4):
        if k == 2:
            plan.set_coeffs(dev(c2[5:9]), 5, 4)
        x = noise(T, B, 700 + k)
        y, yt = run(plan, x, sequential=sequential), run(twin, x, sequential=sequential)
        assert np.array_equal(bits(y[others]), bits(yt[others])), k
        assert (k >= 2) == (not np.array_equal(bits(y[5:9]), bits(yt[5:9]))), k
        if sequential:
            assert np.array_equal(bits(y), bits(eq_reference_f32(x, c1 if k < 2 else mixed, st))), k
    assert np.array_equal(bits(host(plan.state())[others]), bits(host(twin.state())[others]))
    plan.close()
    twin.close()


def test_set_sos_accepts_scipys_layout(gab):
    T, B, S = 6, 128, 3
    coeffs = eq_bank(T, S, 36)
    sos = np.concatenate([coeffs[..., :3], np.ones((T, S, 1), np.float32), coeffs[..., 3:]], axis=-1).astype(np.float64) * 2.0
    a, b = make_plan(gab, T, B, S, coeffs), make_plan(gab, T, B, S)
    b.set_sos(sos)                                      # [T][S][6], a0 = 2 divided out
    x = noise(T, B, 3)
    assert np.array_equal(bits(run(a, x)), bits(run(b, x)))
    b.set_sos(sos[2], tracks=(1, 4))                    # [S][6] for tracks 1..4
    mixed = coeffs.copy()
    mixed[1:5] = coeffs[2]
    a.set_coeffs(dev(mixed))
    assert np.array_equal(bits(run(a, x)), bits(run(b, x)))
    a.close()
    b.close()


@pytest.mark.parametrize("sequential", [False, True])
def test_reset_mid_stream_is_a_fresh_plan(gab, sequential):
    T, B, S = 33, 512, 4
    coeffs = eq_bank(T, S, 37)
    plan, fresh = make_plan(gab, T, B, S, coeffs), make_plan(gab, T, B, S, coeffs)
    for k in range(2):
        run(plan, noise(T, B, 800 + k), sequential=sequential)
    plan.reset()
    assert not host(plan.state()).any()
    for k in range(2):
        x = noise(T, B, 810 + k)
        assert np.array_equal(bits(run(plan, x, sequential=sequential)), bits(run(fresh, x, sequential=sequential)))
    plan.close()
    fresh.close()


def test_scan_and_ordered_form_alternate_on_one_state(gab):
    T, B, S, seed = 128, 512, 8, 38
    coeffs = eq_bank(T, S, seed)
    e_out, e_state, ys, st64 = bank_round_off(T, B, S, seed, coeffs=coeffs, n_buffers=6)
    plan = make_plan(gab, T, B, S, coeffs)
    err = peak = 0.0
    for k in range(6):
        y = run(plan, noise(T, B, 1000 * seed + k), sequential=bool(k & 1))
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    err_state = float(np.abs(host(plan.state()) - st64).max() / np.abs(st64).max())
    plan.close()
    assert err / peak <= tolerance(e_out) and err_state <= tolerance(e_state)


@pytest.mark.parametrize("T,B,S", [(9, 512, 4), (9, 2048, 16), (9, 64, 1), (9, 100, 2)])
def test_a_fresh_plan_is_the_identity(gab, T, B, S):
    plan = make_plan(gab, T, B, S)
    x = noise(T, B, 5)
    assert np.array_equal(bits(run(plan, x)), bits(x))
    assert np.array_equal(bits(run(plan, x, sequential=True)), bits(x))
    plan.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(gab):
    T, B, S = 12, 256, 3
    coeffs = eq_bank(T, S, 41)
    plan, twin = make_plan(gab, T, B, S, coeffs), make_plan(gab, T, B, S, coeffs)
    lib, h = gab.lib, plan._h
    x = noise(T, B, 6)
    run(plan, x)
    run(twin, x)

    def refused(bad, where, call=None):
        with pytest.raises(gab.GabError) as e:
            (call or (lambda: plan.set_coeffs(dev(bad))))()
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
        assert "track %d section %d" % where in str(e.value), str(e.value)

    bad = coeffs.copy(); bad[7, 1, 4] = 1.0                   # a2 = 1: on the triangle's edge
    refused(bad, (7, 1))
    bad = coeffs.copy(); bad[3, 2, 3] = 1.0 + bad[3, 2, 4] + 1e-3; bad[9, 0, 4] = 1.0
    refused(bad, (3, 2))                                      # |a1| > 1 + a2; and the FIRST offender is named
    bad = coeffs.copy(); bad[11, 0, 0] = np.nan
    refused(bad, (11, 0))
    bad = coeffs.copy(); bad[0, 0, 3] = np.inf
    refused(bad, (0, 0))
    bad = coeffs[4:8].copy(); bad[2, 1, 4] = -1.0
    refused(bad, (6, 1), lambda: plan.set_coeffs(dev(bad), 4, 4))
    good = dev(coeffs)
    p = ctypes.c_void_p(good.data_ptr())
    bad_arg = gab._capi.GAB_ERR_INVALID_ARG
    assert lib.gab_eq_set_coeffs(h, None, None) == bad_arg
    assert lib.gab_eq_set_coeffs(None, p, None) == bad_arg
    for first, n in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2**31 - 1, 2)):
        assert lib.gab_eq_set_coeffs_tracks(h, p, first, n, None) == bad_arg, (first, n)
    buf = dev(x.ravel())
    q = ctypes.c_void_p(buf.data_ptr())
    assert lib.gab_eq_process(h, None, q, None) == bad_arg and lib.gab_eq_process(h, q, None, None) == bad_arg
    assert lib.gab_eq_process_sequential(h, None, q, None) == bad_arg
    assert lib.gab_eq_process_batch(h, q, q, 0, None) == bad_arg and lib.gab_eq_process_batch(h, q, q, -3, None) == bad_arg
    assert lib.gab_eq_process_batch(h, None, q, 1, None) == bad_arg
    assert lib.gab_eq_state(h, None, None) == bad_arg and lib.gab_eq_form(h, None, None) == bad_arg
    assert lib.gab_eq_reset(None, None) == bad_arg
    # the old coefficients are still in force, the state untouched
    x = noise(T, B, 7)
    assert np.array_equal(bits(run(plan, x)), bits(run(twin, x)))
    assert np.array_equal(bits(host(plan.state())), bits(host(twin.state())))
    plan.close()
    twin.close()


# ---- 6. worth having ------------------------------------------------------------------------------------------
def test_one_fused_launch_beats_eight_iir_launches(gab, orc):
    """8192 x 512, eight sections: the median device time of gab_eq_process is below that of the parent's way of doing
    it, eight gab_iir launches over the same block — measured here, alternating.  A floor, not the target
    (tools/eq_bench.py reports the ratio)."""
    import torch
    T, B, S = 8192, 512, 8
    plan = make_plan(gab, T, B, S, eq_bank(T, S, 51))
    x = dev(noise(T, B, 8).ravel())
    y = torch.empty_like(x)
    c = orc.iir_coeffs(0.25)
    st = dev(np.zeros(2 * T, np.float32))

    def eq():
        plan.process(x, out=y)

    z = torch.empty_like(x)
    cc = (ctypes.c_float * 5)(*[float(v) for v in c])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    z2 = torch.empty_like(x)
    px, pz, pz2, pst = (ctypes.c_void_p(t.data_ptr()) for t in (x, z, z2, st))

    def iir8():                      # x -> z -> z2 -> z ...: eight passes over the block, nothing allocated
        src = px
        for i in range(S):
            dst = (pz, pz2)[i & 1]
            gab.check(gab.lib.gab_iir(src, dst, cc, pst, T, B, stream))
            src = dst

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for _ in range(10):
        eq()
        iir8()
    torch.cuda.synchronize()
    t_eq, t_iir = [], []
    for _ in range(50):
        t_eq.append(timed(eq))
        t_iir.append(timed(iir8))
    m_eq, m_iir = float(np.median(t_eq)), float(np.median(t_iir))
    print("8192 x 512, 8 sections: gab_eq_process %.1f us, eight gab_iir launches %.1f us (x%.2f)" % (m_eq, m_iir, m_iir / m_eq))
    plan.close()
    assert m_eq < m_iir, (m_eq, m_iir)
