"""The equaliser plan (gab_eq_*) on the device.

Ordered form (eq_sequential_kernel): bit for bit against eq_reference_f32 (tests/test_eq_host.py).
Scan form (eq_scan_kernel): against float64 (scipy's sosfilt on the float32 coefficients), outputs and final state,
within max(1e-5, 4 e32) of the float64 peak per case, where e32 is what eq_reference_f32 itself loses against float64
on the same inputs (computed here on the CPU; at 16 384 tracks on the first 64).  Held on two banks: eq_bank (240 Hz and
up, e32 <= 1e-4) and eq_bank_low (20-240 Hz at 48 and 96 kHz, Q up to 30: e32 7e-4 .. 1.2e-2, the carried state hundreds
of times the signal), whose cases test_eq_host.py has shown the scan's arithmetic itself to pass.
1e-5 of peak is the project's rule for
re-associated float32 paths (test_iir_wave_scan_with_carried_state); the factor 4 allows for the rounding of the table
and of six combine steps on top of a recursion whose own round-off may already exceed 1e-5.  The state is held to the
same rule with its own e32 and its own peak.  Every case prints its figures and err / e32 (pytest -s).
"""
import ctypes

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_eq_host import (LOW_CASES, LOW_T, N_BUFFERS, SCAN_CASES, bank_round_off, case_seed, eq_bank, eq_bank_low, eq_form,
                          eq_reference_f32, low_case, low_seed, noise)

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


# ---- 2a. the low band: rumble filters, shelves and hum notches at 48 and 96 kHz ---------------------------------
@pytest.mark.parametrize("B,S,fs", LOW_CASES)
def test_scan_form_against_float64_low_band(gab, B, S, fs):
    """test_scan_form_against_float64 on eq_bank_low: the same rule, max(1e-5, 4 e32), with the low bank's own e32."""
    coeffs, e_out, e_state, ys, st64 = low_case(B, S, fs)
    seed = low_seed(B, S, fs)
    plan = make_plan(gab, LOW_T, B, S, coeffs)
    assert plan.form != (0, 0) and plan.form == eq_form(B, S)
    err = peak = 0.0
    for k in range(N_BUFFERS):
        y = run(plan, noise(LOW_T, B, 1000 * seed + k))
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    err /= peak
    err_state = float(np.abs(host(plan.state()) - st64).max() / np.abs(st64).max())
    print("eq scan low band B=%d S=%d fs=%d form=%s: outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (B, S, fs, plan.form, err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    plan.close()
    assert err <= tolerance(e_out), (err, e_out)
    assert err_state <= tolerance(e_state), (err_state, e_state)


@pytest.mark.parametrize("B,S,fs", [(64, 4, 96000), (512, 16, 48000), (2048, 4, 96000)])
def test_ordered_form_bit_for_bit_low_band(gab, B, S, fs):
    coeffs = low_case(B, S, fs)[0]
    plan = make_plan(gab, LOW_T, B, S, coeffs)
    st = np.zeros((LOW_T, S, 2), np.float32)
    for k in range(3):
        x = noise(LOW_T, B, 70 + k)
        y = run(plan, x, sequential=True)
        ref = eq_reference_f32(x, coeffs, st)
        assert np.array_equal(bits(y), bits(ref)), k
        assert np.array_equal(bits(host(plan.state())), bits(st)), k
    plan.close()


@pytest.mark.parametrize("B,S,fs", [(64, 4, 96000), (2048, 4, 96000)])
def test_batch_and_alternation_on_the_low_bank(gab, B, S, fs):
    """One launch over twelve buffers is twelve launches, bit for bit; scan and ordered calls alternating on one state
    stay within the rule -- on the bank where the state handed from one form to the other is hundreds of times the
    signal."""
    coeffs, e_out, e_state, ys, st64 = low_case(B, S, fs)
    seed = low_seed(B, S, fs)
    xs = np.stack([noise(LOW_T, B, 1000 * seed + k) for k in range(N_BUFFERS)])
    a, b, c = (make_plan(gab, LOW_T, B, S, coeffs) for _ in range(3))
    singles = np.stack([run(a, xs[k]) for k in range(N_BUFFERS)])
    batch = host(b.process_batch(dev(xs.ravel()))).reshape(xs.shape)
    assert np.array_equal(bits(batch), bits(singles))
    assert np.array_equal(bits(host(a.state())), bits(host(b.state())))
    err = peak = 0.0
    for k in range(N_BUFFERS):
        y = run(c, xs[k], sequential=bool(k & 1))
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    err /= peak
    err_state = float(np.abs(host(c.state()) - st64).max() / np.abs(st64).max())
    print("eq scan/ordered alternating, low band B=%d S=%d fs=%d: outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (B, S, fs, err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    for p in (a, b, c):
        p.close()
    assert err <= tolerance(e_out), (err, e_out)
    assert err_state <= tolerance(e_state), (err_state, e_state)


def _pole_radius(row):
    return max(float(np.abs(np.roots([1.0, float(a1), float(a2)])).max()) for a1, a2 in np.asarray(row)[:, 3:])


SINE_GAIN_TOLERANCE = 4 * 1.03e-4


def test_steady_state_gain_is_the_transfer_function(gab):
    """A check that shares no recursion with scipy or eq_cascade: a settled sine comes out with the gain
    |prod B(e^jw) / A(e^jw)|, evaluated in float64 from the float32 coefficients.  One 4-section low-bank row
    (48 kHz, seed 7: high-pass, shelf, two peaking sections; slowest pole radius 0.99962), sines of amplitude 0.5 at
    30, 100 and 1000 Hz on three tracks, 512-sample buffers: 84 buffers to let the transient fall to 1e-7
    (ln 1e-7 / ln r samples), then the rms gain over 75 buffers = 38 400 samples, whole periods of all three.
    The bound is relative and the same for the three: four times what the ordered float32 cascade itself misses the
    transfer function by on this input, measured on the CPU (eq_reference_f32): +1.03e-4 at 30 Hz, -5.0e-6 at 100 Hz,
    +9.7e-7 at 1 kHz (float64: below 1e-10, so the settling and the window contribute nothing); its worst, 1.03e-4,
    is the figure -- the rounding noise of the row is broadband, not a property of the one frequency."""
    fs, B, window = 48000, 512, 75
    row = eq_bank_low(1, 4, 7, fs)[0]
    freqs = np.array([30.0, 100.0, 1000.0])
    n_settle = int(np.ceil(np.log(1e-7) / np.log(_pole_radius(row)) / B))
    assert 10 <= n_settle <= 200, n_settle
    nb = n_settle + window
    x = (0.5 * np.sin(2 * np.pi * freqs[:, None] * np.arange(nb * B)[None, :] / fs)).astype(np.float32).reshape(3, nb, B)
    z = np.exp(-2j * np.pi * freqs / fs)
    c = row.astype(np.float64)
    gain = np.abs(np.prod([(c[s, 0] + c[s, 1] * z + c[s, 2] * z * z) / (1 + c[s, 3] * z + c[s, 4] * z * z) for s in range(4)], axis=0))
    rms_in = np.sqrt((x[:, n_settle:].astype(np.float64) ** 2).mean(axis=(1, 2)))
    coeffs = np.broadcast_to(row, (3, 4, 5)).copy()
    for sequential in (False, True):
        plan = make_plan(gab, 3, B, 4, coeffs)
        assert plan.form == (8, 1)
        ys = [run(plan, x[:, k], sequential=sequential) for k in range(nb)][n_settle:]
        plan.close()
        got = np.sqrt((np.stack(ys, axis=1).astype(np.float64) ** 2).mean(axis=(1, 2))) / rms_in
        rel = got / gain - 1
        print("eq steady-state gain, %s form: expected %s, relative error %s (bound %.3g)"
              % ("ordered" if sequential else "scan", gain, rel, SINE_GAIN_TOLERANCE))
        assert (np.abs(rel) <= SINE_GAIN_TOLERANCE).all(), (sequential, rel)


def test_a_tail_through_subnormals_ordered_form(gab):
    """One buffer of noise, then silence until the float32 reference's state is subnormal or zero everywhere: the
    ordered kernel keeps every subnormal the reference keeps (one rounding per operation: no flush to zero), outputs
    and state, bit for bit in every buffer.  The scan form over the same tail stays finite and ends at zero or at
    subnormals."""
    T, S, B = 5, 3, 100
    tiny = np.finfo(np.float32).tiny
    coeffs = eq_bank(T, S, 4)
    plan = make_plan(gab, T, B, S, coeffs)
    assert plan.form == (0, 0)
    st = np.zeros((T, S, 2), np.float32)
    x, zero = noise(T, B, 90), np.zeros((T, B), np.float32)
    n = subnormal_outputs = 0
    while n == 0 or (np.abs(st) >= tiny).any():
        assert n < 1000, "the tail does not die"
        xin = x if n == 0 else zero
        ref = eq_reference_f32(xin, coeffs, st)
        subnormal_outputs += int(((ref != 0) & (np.abs(ref) < tiny)).sum())
        assert np.array_equal(bits(run(plan, xin)), bits(ref)), n
        assert np.array_equal(bits(host(plan.state())), bits(st)), n
        n += 1
    plan.close()
    subnormal_states = int(((st != 0) & (np.abs(st) < tiny)).sum())
    print("eq tail: %d buffers of %d, %d subnormal outputs, %d subnormal state words at the end" % (n, B, subnormal_outputs, subnormal_states))
    assert subnormal_outputs > 1000 and subnormal_states > 0
    # the scan form: the same filters and noise, 10 % more silence than the ordered form needed
    B2 = 128
    plan = make_plan(gab, T, B2, S, coeffs)
    assert plan.form == (2, 1)
    x2 = np.zeros((T, B2), np.float32)
    x2[:, :B] = x
    assert np.isfinite(run(plan, x2)).all()
    zero = np.zeros((T, B2), np.float32)
    for k in range(int(np.ceil(1.1 * n * B / B2))):
        assert np.isfinite(run(plan, zero)).all(), k
    end = host(plan.state())
    plan.close()
    assert np.isfinite(end).all() and (np.abs(end) < tiny).all(), end


@pytest.mark.parametrize("B,sequential", [(256, False), (100, True)])
def test_a_nan_stays_in_its_track(gab, B, sequential):
    """A NaN in track 64 and an infinity in track 129 of 130 (64-track workgroups of the ordered kernel plus a
    remainder; 4-track workgroups of the scan), in buffer 1 of 3: every other track has the bits of the run without
    them, the two tracks are non-finite from that sample on, state included, and reset() gives a fresh plan."""
    T, S, at = 130, 4, 37
    coeffs = eq_bank(T, S, 61)
    clean, dirty, fresh = (make_plan(gab, T, B, S, coeffs) for _ in range(3))
    assert clean.form == ((4, 1) if B == 256 else (0, 0))
    hit = np.array([64, 129])
    others = np.setdiff1d(np.arange(T), hit)
    for k in range(3):
        x = noise(T, B, 900 + k)
        yc = run(clean, x, sequential=sequential)
        if k == 1:
            x[64, at], x[129, at] = np.nan, np.inf
        yd = run(dirty, x, sequential=sequential)
        assert np.array_equal(bits(yd[others]), bits(yc[others])), k
        if k == 0:
            assert np.array_equal(bits(yd), bits(yc))
        else:
            assert not np.isfinite(yd[hit, at if k == 1 else 0:]).any(), k
    sc, sd = host(clean.state()), host(dirty.state())
    assert np.array_equal(bits(sd[others]), bits(sc[others]))
    assert not np.isfinite(sd[hit]).any()
    dirty.reset()
    assert not host(dirty.state()).any()
    for k in range(2):
        x = noise(T, B, 910 + k)
        assert np.array_equal(bits(run(dirty, x, sequential=sequential)), bits(run(fresh, x, sequential=sequential)))
    for p in (clean, dirty, fresh):
        p.close()


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
