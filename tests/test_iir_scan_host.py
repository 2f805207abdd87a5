"""gab_iir's wave scan (iir_scan_kernel, k_recursive.hip) without a GPU: the bank of sections the scan is held to,
the form gab_iir dispatches, and the kernel's arithmetic restated in numpy float32.

    IIR_BANK           single sections {b0,b1,b2,a1,a2} as float32: the two filters the suite always used (poles at
                       radius 0.41 and 0.85), what a channel strip carries below 240 Hz at 48 and 96 kHz (poles next to
                       z = 1, the DF-II state hundreds to thousands of times the signal), a mid-band bell, a bell
                       at 18 kHz, and the other end: bells and a cut at 20-23 kHz and the z -> -z mirror image of
                       the 30 Hz high-pass (poles next to z = -1, z1 ~ -z2).
    iir_form           (M, H) of the scan gab_iir launches for (tracks, bufsize); (0, 0): the ordered kernel.
    iir_scan_emulated  iir_scan_kernel<M, H> operation for operation: the local pass and the output taps one rounding
                       per operation, the combine steps and the correction with fused multiply-adds (not the
                       device's bits there: _fmaf rounds twice).  Never a GPU test's expected value: it says, without
                       a GPU, what the ALGORITHM loses on a section, so that a failure on the device is the device
                       code's.

The rule is the equaliser's, unchanged (test_eq_host.py, test_eq_gpu.py): outputs and final state within
max(1e-5, 4 e32) of the float64 peak, e32 being what the ordered float32 form itself loses against float64 on the same
input.  The scan runs on (u, d) = (z1, z1 - sg z2), sg = -1 for a1 > 0 (scan_sign).  On (z1, z2), its first form, a section with poles near z = 1 has
A^n ~ [n+1 -n; n -(n-1)] acting on z1 ~ z2: measured on the device at 16 to 44 600 times e32 from the 1 kHz bell down to
the 20 Hz high-pass (profiles/r16_iir_scan_band.txt; test_the_z_basis_is_what_failed keeps that arithmetic, and shows
that this file notices it).
Figures of every case: pytest -s.
"""
import numpy as np
import pytest

from test_eq_host import (N_BUFFERS, _fmaf, _rbj_highpass, _rbj_lowshelf, _rbj_peaking, _shfl_up, eq_cascade,
                          eq_reference_f32, eq_reference_f64, noise)

C2 = np.array([0.2, 0.1, -0.05, -1.2, 0.72], np.float32)           # test_gpu_parity.py's second filter
# orc.iir_coeffs(0.25), the reference's own filter (test_the_bank_is_stable_and_what_it_says checks the bits)
REFERENCE = np.array([0x3E95F3B2, 0x3F15F3B2, 0x3E95F3B2, 0x335BEFA6, 0x3E2F9D96], np.uint32).view(np.float32)


def _section(sec):
    """a0 divided out in float64, rounded once (eq_bank's way)."""
    return (sec[[0, 1, 2, 4, 5]] / sec[3]).astype(np.float32)


IIR_BANK = [
    ("reference", REFERENCE),
    ("c2", C2),
    ("hp20", _section(_rbj_highpass(20.0, 0.7071, 48000.0))),
    ("hp30", _section(_rbj_highpass(30.0, 0.7071, 48000.0))),
    ("hp80", _section(_rbj_highpass(80.0, 0.7071, 48000.0))),
    ("hp240", _section(_rbj_highpass(240.0, 0.7071, 48000.0))),
    ("hp20_96k", _section(_rbj_highpass(20.0, 0.7071, 96000.0))),
    ("shelf100", _section(_rbj_lowshelf(100.0, 9.0, 48000.0))),
    ("bell50_q30", _section(_rbj_peaking(50.0, 30.0, 6.0, 48000.0))),
    ("notch60_q30", _section(_rbj_peaking(60.0, 30.0, -24.0, 48000.0))),
    ("bell1k", _section(_rbj_peaking(1000.0, 2.0, 6.0, 48000.0))),
    ("bell18k", _section(_rbj_peaking(18000.0, 8.0, 6.0, 48000.0))),
    ("bell20k_q30", _section(_rbj_peaking(20000.0, 30.0, 6.0, 48000.0))),
    ("bell22k", _section(_rbj_peaking(22000.0, 8.0, 6.0, 48000.0))),
    ("cut23k", _section(_rbj_peaking(23000.0, 2.0, -12.0, 48000.0))),
    ("hp30_mirror", _section(_rbj_highpass(30.0, 0.7071, 48000.0)) * np.array([1, -1, 1, -1, 1], np.float32)),
]
BANK = dict(IIR_BANK)
BANK_NAMES = [name for name, _ in IIR_BANK]
HIGH_NAMES = ["bell20k_q30", "bell22k", "cut23k", "hp30_mirror"]     # poles next to z = -1: the low entries' mirror image
LOW_NAMES = [n for n in BANK_NAMES if n not in ["reference", "c2", "bell1k", "bell18k"] + HIGH_NAMES]
# every instantiation gab_iir has, as (B, M, H)
FORMS = [(64, 1, 1), (128, 2, 1), (256, 4, 1), (512, 8, 1), (1024, 16, 1), (512, 4, 2), (1024, 4, 4)]
HOST_T = 8


def is_stable(c):
    """The equaliser's check (eq_consts_kernel), which gab_iir applies on the host: finite and inside the triangle."""
    c = np.asarray(c, np.float32).astype(np.float64)
    return bool(np.isfinite(c).all() and abs(c[4]) < 1.0 and abs(c[3]) < 1.0 + c[4])


def iir_form(tracks, bufsize):
    """(M, H) of the scan gab_iir launches on 16-byte aligned buffers and a stable, finite section; (0, 0): none."""
    m = bufsize // 64
    if bufsize % 64 or m not in (1, 2, 4, 8, 16):
        return 0, 0
    if m >= 8 and tracks >= 16384:
        return 4, m // 4
    return m, 1


def scan_sign(c):
    """sg of the scan's basis (u, d) = (z1, z1 - sg z2): +1 for a1 <= 0 (poles in the right half plane, z1 ~ z2 near
    z = 1), -1 for a1 > 0 (z1 ~ -z2 near z = -1)."""
    return -1.0 if np.float32(np.asarray(c, np.float32)[3]) > 0 else 1.0


def iir_scan_consts(c, M, basis="ud"):
    """(alpha [M], beta [M], p [6][4]) in float64, not yet rounded: make_scan_consts' arithmetic on the float32
    coefficients.  basis "ud": as they act on (u, d) = (z1, z1 - z2), formed from the (z1, z2) powers
    (eq_consts_kernel's arithmetic); "z": on (z1, z2) themselves, the scan's first form."""
    c = np.asarray(c, np.float32).astype(np.float64)
    sg = scan_sign(c)
    A0, A1 = -c[3], -c[4]
    P0, P1, P2, P3 = 1.0, 0.0, 0.0, 1.0
    alpha, beta, p = np.empty(M), np.empty(M), np.empty((6, 4))
    for i in range(M):                      # P = A P = A^(i+1); its first row is w[i]'s response to (z1, z2)
        P0, P1, P2, P3 = A0 * P0 + A1 * P2, A0 * P1 + A1 * P3, P0, P1
        alpha[i], beta[i] = (P0 + sg * P1, -sg * P1) if basis == "ud" else (P0, P1)
    for q in range(6):
        if basis == "ud":                   # T P T^-1, T = [1 0; 1 -sg], T^-1 = [1 0; sg -sg]
            p[q] = P0 + sg * P1, -sg * P1, (P0 + sg * P1) - sg * (P2 + sg * P3), P3 - sg * P1
        else:
            p[q] = P0, P1, P2, P3
        P0, P1, P2, P3 = P0 * P0 + P1 * P2, P0 * P1 + P1 * P3, P2 * P0 + P3 * P2, P2 * P1 + P3 * P3
    return alpha, beta, p


def iir_scan_emulated(x, c, state, M, H, dtype=np.float32, basis="ud"):
    """iir_scan_kernel<M, H> in numpy, vectorised over tracks and lanes: x [T][64 M H], c the shared section [5],
    state [T][2] = (z1, z2) of `dtype`, updated in place.  Steps 1 and 4 are one numpy operation in `dtype` per
    operation: one rounding each, in the kernel's order (the kernel is built without contraction).  Steps 2 and 3 are
    the kernel's fmaf (basis "z", the scan's first form, had none).  The constants are formed in float64 and rounded
    once to `dtype`.  dtype float64: the same algorithm with nothing rounded to float32."""
    T, B = x.shape
    assert B == 64 * M * H and state.shape == (T, 2) and state.dtype == dtype
    b0, b1, b2, a1, a2 = (dtype(v) for v in np.asarray(c, np.float32))
    alpha, beta, p = (k.astype(dtype) for k in iir_scan_consts(c, M, basis))
    xs = np.array(x, dtype).reshape(T, H, 64, M)
    y = np.empty((T, H, 64, M), dtype)
    lanes = np.arange(64)
    if basis == "ud" and dtype == np.float32:
        fma = _fmaf
    else:
        def fma(a, b, c):
            return c + a * b
    in1, in2 = state[:, 0].copy(), state[:, 1].copy()
    for h in range(H):
        z1, z2 = np.zeros((T, 64), dtype), np.zeros((T, 64), dtype)
        z1[:, 0], z2[:, 0] = in1, in2
        w = np.empty((T, 64, M), dtype)
        for i in range(M):                                       # 1. local pass
            wv = (xs[:, h, :, i] - a1 * z1) - a2 * z2
            z2, z1 = z1, wv
            w[:, :, i] = wv
        e1, e2 = z1, (z1 - dtype(scan_sign(c)) * z2 if basis == "ud" else z2)      # 2. the scan of the outgoing states
        for q in range(6):
            d = 1 << q
            u1, u2 = _shfl_up(e1, d), _shfl_up(e2, d)
            if basis == "ud":
                n1 = fma(p[q, 1], u2, fma(p[q, 0], u1, e1))
                n2 = fma(p[q, 3], u2, fma(p[q, 2], u1, e2))
            else:
                n1 = e1 + (p[q, 0] * u1 + p[q, 1] * u2)
                n2 = e2 + (p[q, 2] * u1 + p[q, 3] * u2)
            e1, e2 = np.where(lanes >= d, n1, e1), np.where(lanes >= d, n2, e2)
        s1, s2 = _shfl_up(e1, 1), _shfl_up(e2, 1)
        s1[:, 0] = s2[:, 0] = 0.0
        for i in range(M):                                       # 3. homogeneous correction
            if basis == "ud":
                w[:, :, i] = fma(beta[i], s2, fma(alpha[i], s1, w[:, :, i]))
            else:
                w[:, :, i] = w[:, :, i] + (alpha[i] * s1 + beta[i] * s2)
        p1 = _shfl_up(w[:, :, M - 1], 1)                         # 4. output taps
        p2 = _shfl_up(w[:, :, M - 2], 1) if M >= 2 else _shfl_up(w[:, :, 0], 2)
        p1[:, 0], p2[:, 0] = in1, in2
        if M == 1:
            p2[:, 1] = in1
        for i in range(M):
            wm1 = w[:, :, i - 1] if i >= 1 else p1
            wm2 = w[:, :, i - 2] if i >= 2 else (p1 if i == 1 else p2)
            y[:, h, :, i] = (b0 * w[:, :, i] + b1 * wm1) + b2 * wm2
        in1, in2 = w[:, 63, M - 1].copy(), (w[:, 63, M - 2] if M >= 2 else p1[:, 63]).copy()
    state[:, 0], state[:, 1] = in1, in2
    assert y.dtype == dtype
    return y.reshape(T, B)


def bank_seed(name, B):
    return 100 * BANK_NAMES.index(name) + B // 64


def iir_reference(c, xs):
    """What the ordered forms give on the buffers xs (each [n][B], one shared section c): (e32 of the outputs, e32 of
    the DF-II state, y64 per buffer, final float64 DF-II state [n][2], y32 per buffer, final float32 state [n][2]).
    y64 is scipy's sosfilt in float64 on the float32 coefficients (eq_reference_f64); e32 is eq_reference_f32's miss
    against it, peak-normalised over the whole run; the float64 DF-II state comes from eq_cascade in float64, which is
    checked against sosfilt on the way (bank_round_off's arithmetic, on given inputs)."""
    n = xs[0].shape[0]
    coeffs = np.broadcast_to(np.asarray(c, np.float32), (n, 1, 5)).copy()
    st32, st64, zi = np.zeros((n, 1, 2), np.float32), np.zeros((n, 1, 2), np.float64), np.zeros((n, 1, 2), np.float64)
    err = peak = 0.0
    y64s, y32s = [], []
    for x in xs:
        y32 = eq_reference_f32(x, coeffs, st32)
        y64 = eq_reference_f64(x, coeffs, zi)
        yc = eq_cascade(x.astype(np.float64), coeffs.astype(np.float64), st64, np.float64)
        assert np.abs(yc - y64).max() <= 1e-9 * max(np.abs(y64).max(), 1.0)
        err = max(err, float(np.abs(y32 - y64).max()))
        peak = max(peak, float(np.abs(y64).max()))
        y64s.append(y64)
        y32s.append(y32)
    e_state = float(np.abs(st32 - st64).max() / np.abs(st64).max())
    return err / peak, e_state, y64s, st64[:, 0], y32s, st32[:, 0]


_host_cases = {}


def host_case(name, B):
    """(inputs, iir_reference's result) of a bank entry at HOST_T tracks and N_BUFFERS buffers of B samples of uniform
    noise; made once per process (the forms that share a buffer size share it) and read-only."""
    if (name, B) not in _host_cases:
        xs = [noise(HOST_T, B, 1000 * bank_seed(name, B) + k) for k in range(N_BUFFERS)]
        ref = iir_reference(BANK[name], xs)
        for a in xs + ref[2] + ref[4] + [ref[3], ref[5]]:
            a.flags.writeable = False
        _host_cases[(name, B)] = (xs, ref)
    return _host_cases[(name, B)]


def scan_errors(ys, state, ref):
    """(err of the outputs, err of the state) against iir_reference's float64, by its yardsticks."""
    _, _, y64s, st64 = ref[:4]
    err = max(float(np.abs(y - y64).max()) for y, y64 in zip(ys, y64s))
    peak = max(float(np.abs(y64).max()) for y64 in y64s)
    return err / peak, float(np.abs(state - st64).max() / np.abs(st64).max())


def emulation_errors(name, B, M, H, basis="ud"):
    xs, ref = host_case(name, B)
    st = np.zeros((HOST_T, 2), np.float32)
    ys = [iir_scan_emulated(x, BANK[name], st, M, H, basis=basis) for x in xs]
    return scan_errors(ys, st, ref)


def rule(e32):
    return max(1e-5, 4.0 * e32)


# ---------------------------------------------------------------------------
def test_the_bank_is_stable_and_what_it_says(orc):
    assert np.array_equal(REFERENCE.view(np.uint32), orc.iir_coeffs(0.25).view(np.uint32))
    assert len(IIR_BANK) == 16 and len(BANK) == 16
    radius = {}
    for name, c in IIR_BANK:
        assert c.dtype == np.float32 and c.shape == (5,) and is_stable(c), name
        radius[name] = float(np.abs(np.roots([1.0, float(c[3]), float(c[4])])).max())
        assert radius[name] < 1.0, name
    assert abs(radius["reference"] - 0.41) < 0.01 and abs(radius["c2"] - 0.85) < 0.01
    for name in LOW_NAMES:                      # poles next to z = 1 ...
        c = BANK[name].astype(np.float64)
        assert radius[name] > 0.97 and 1.0 + c[3] + c[4] < 1e-3, name
    c = BANK["bell18k"].astype(np.float64)      # ... towards z = -1, a1 > 0 ...
    assert c[3] > 1.0 and radius["bell18k"] > 0.9 and np.roots([1.0, c[3], c[4]]).real.max() < -0.5
    for name in HIGH_NAMES:                     # ... and next to it: A(-1) = 1 - a1 + a2 small, as A(1) is for the low entries
        c = BANK[name].astype(np.float64)
        assert radius[name] > 0.93 and c[3] > 1.7 and 1.0 - c[3] + c[4] < 0.3 and scan_sign(BANK[name]) == -1.0, name
    m, o = BANK["hp30_mirror"], BANK["hp30"]
    assert np.array_equal(m[[0, 2, 4]], o[[0, 2, 4]]) and np.array_equal(m[[1, 3]], -o[[1, 3]]) and 1.0 - float(m[3]) + float(m[4]) < 1e-3
    assert all(scan_sign(BANK[n]) == 1.0 for n in LOW_NAMES + ["c2", "bell1k"]) and scan_sign(BANK["bell18k"]) == -1.0
    for bad in ([1, 0, 0, 0, 1.01], [1, 0, 0, np.nan, 0.5], [np.inf, 0, 0, 0, 0.5], [1, 0, 0, 1.6, 0.5], [1, 0, 0, 0, -1.0]):
        assert not is_stable(np.array(bad, np.float32)), bad


def test_iir_form():
    for B, M, H in FORMS:
        assert iir_form(16384 if H > 1 else 12, B) == (M, H)
    assert iir_form(16383, 512) == (8, 1) and iir_form(16383, 1024) == (16, 1)
    assert iir_form(70000, 256) == (4, 1) and iir_form(70000, 64) == (1, 1)
    for B in (1, 63, 100, 192, 320, 513, 2048, 4096):
        assert iir_form(12, B) == (0, 0) and iir_form(20000, B) == (0, 0), B


def test_the_emulated_scan_is_the_kernels_algorithm():
    """On the reference's filter the emulation agrees with the ordered float32 form within 1e-6 of peak (the device:
    ~1e-7, test_iir_wave_scan_with_carried_state); in float64 with unrounded constants it is the float64 filter to
    1e-9 of peak, so the cut into lanes, the six combine steps, the correction, the taps and the hand-over of the state
    between segments and buffers are the recurrence's own, in both bases, over all twelve buffers.  The entries with
    poles next to z = 1 or z = -1 are held to 1e-5 there: their constants come from powers with entries in the
    hundreds that cancel to 1e-3, which costs float64 constants some 1e-10 of their value, and a state up to 1e6 times
    the output makes that 1e-6 of peak (measured: 2.7e-6 on the 20 Hz high-pass at 96 kHz) -- nothing beside float32's
    6e-8 per constant, and still far below those entries' own float32 round-off (2e-4 and up) and anything a
    misplaced tap or power would give."""
    for B, M, H in FORMS:
        xs, ref = host_case("reference", B)
        st = np.zeros((HOST_T, 2), np.float32)
        for k, x in enumerate(xs):
            y = iir_scan_emulated(x, REFERENCE, st, M, H)
            assert np.abs(y - ref[4][k]).max() <= 1e-6 * np.abs(ref[4][k]).max(), (B, M, H, k)
        assert np.abs(st - ref[5]).max() <= 1e-6 * np.abs(ref[5]).max(), (B, M, H)
    for name in BANK_NAMES:
        bound = 1e-5 if name in LOW_NAMES + HIGH_NAMES else 1e-9
        for B, M, H in FORMS:
            xs, ref = host_case(name, B)
            for basis in ("ud", "z"):
                st = np.zeros((HOST_T, 2), np.float64)
                ys = [iir_scan_emulated(x, BANK[name], st, M, H, np.float64, basis) for x in xs]
                err, err_state = scan_errors(ys, st, ref)
                assert err <= bound and err_state <= bound, (name, B, M, H, basis, err, err_state)


@pytest.mark.parametrize("B,M,H", FORMS)
@pytest.mark.parametrize("name", BANK_NAMES)
def test_scan_emulation_is_within_the_rule(name, B, M, H):
    """The scan's ALGORITHM against float64, every bank entry in every form gab_iir has: outputs and final state
    within max(1e-5, 4 e32).  That makes the bank one the device can be held to (test_iir_scan_gpu.py)."""
    e_out, e_state = host_case(name, B)[1][:2]
    err, err_state = emulation_errors(name, B, M, H)
    print("iir scan emulated %s B=%d form=(%d, %d): outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (name, B, M, H, err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    assert err <= rule(e_out), (err, e_out)
    assert err_state <= rule(e_state), (err_state, e_state)


def test_the_z_basis_is_what_failed():
    """The same scan on (z1, z2), as gab_iir first had it: fine on the two filters the suite used, outside the rule
    from the mid-band bell down, and returning noise for a rumble filter.  This file's rule notices it."""
    for name in ("reference", "c2"):
        err, _ = emulation_errors(name, 512, 8, 1, basis="z")
        assert err <= rule(host_case(name, 512)[1][0]), name
    for name, B, M, H, least in (("bell1k", 512, 8, 1, 5.0), ("hp240", 256, 4, 1, 20.0), ("hp30", 512, 8, 1, 1000.0),
                                 ("bell50_q30", 1024, 16, 1, 1000.0), ("hp20_96k", 1024, 4, 4, 1000.0)):
        e_out = host_case(name, B)[1][0]
        err, _ = emulation_errors(name, B, M, H, basis="z")
        print("iir scan emulated on (z1, z2) %s B=%d form=(%d, %d): outputs %.3g of peak (e32 %.3g, ratio %.0f)"
              % (name, B, M, H, err, e_out, err / e_out))
        assert err > rule(e_out) and err > least * e_out, (name, err, e_out)
