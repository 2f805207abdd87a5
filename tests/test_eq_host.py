"""The equaliser plan (gab_eq_*) without a GPU: the references the GPU tests compare against, shown to be what they
claim to be; the test banks, shown to be usable; argument checks and exports.

    eq_reference_f32   the ordered float32 cascade, one rounding per operation, in the golden's order
                       (w = (x - a1*z1) - a2*z2; y = (b0*w + b1*z1) + b2*z2): what eq_sequential_kernel must equal
                       bit for bit.  With one section it reproduces the pinned oracle's iir bit for bit.
    eq_reference_f64   scipy.signal.sosfilt in float64 on the float32-rounded coefficients, zi carried across buffers:
                       the truth the scan form is measured against.
    eq_cascade         the same DF-II recurrence in any dtype; in float64 it gives the DF-II state (z1, z2) that
                       sosfilt, a transposed form, does not have, and is checked here against sosfilt.
    eq_bank            the test banks: section 0 a 12 dB/oct high-pass at fmin..4 fmin, the others RBJ peaking sections.

The banks' own float32 round-off (eq_reference_f32 against eq_reference_f64, peak-normalised, 12 buffers of uniform
noise) is the yardstick the GPU tolerances are derived from (max(1e-5, 4 e32) per case, see test_eq_gpu.py).  A bank whose
own error exceeds 1e-4 of peak tests DF-II round-off, not the kernel.  Measured here (T = 128, B = 512, seed 7;
e32 of the outputs for S = 1, 4, 8, 16):

    fmin =  20 Hz:  1.5e-03  6.3e-04  6.7e-04  5.8e-04     (not usable: a float32 DF-II high-pass at 20..80 Hz)
    fmin =  80 Hz:  2.5e-04  8.3e-05  1.2e-04  1.4e-04
    fmin = 160 Hz:  6.6e-05  2.0e-05  4.9e-05  6.4e-05
    fmin = 240 Hz:  3.0e-05  1.2e-05  3.2e-05  3.2e-05     over all of SCAN_CASES: 6.0e-06 .. 8.0e-05

so FMIN = 240 Hz (the error goes with about 1 / fmin^2; 160 Hz leaves no margin for the larger banks).  The figures
of every case: pytest -s.

    eq_bank_low        what a channel strip carries, at 48 and 96 kHz: section 0 a high-pass at 20..80 Hz, section 1 a low
                       shelf at 60..200 Hz, the others peaking sections and notches at 20..240 Hz with Q up to 30.
    eq_scan_emulated   eq_scan_kernel's arithmetic in numpy float32 (not its bits: fmaf is rounded twice here).  Never a
                       GPU test's expected value: it shows, without a GPU, that the scan's algorithm passes the rule on
                       a bank, so that a failure on the device is the device code's.

The low bank is far outside that 1e-4, on purpose: the scan is held to max(1e-5, 4 e32) of ITS e32 there.  Measured here
(LOW_CASES: T = 24, seed B + S + fs / 48000; e32 of the outputs at B = 64, 128, 256, 512, 1024, 2048):

    48 kHz, S = 1:   7.3e-04  1.3e-03  1.4e-03  1.5e-03  1.6e-03  1.5e-03
    48 kHz, S = 4:   7.5e-04  8.2e-04  7.0e-04  1.8e-03  1.7e-03  3.7e-03     S = 16: 3.0e-03 (512), 4.3e-03 (2048)
    96 kHz, S = 1:   1.4e-03  2.8e-03  3.1e-03  3.2e-03  4.9e-03  6.0e-03
    96 kHz, S = 4:   1.5e-03  2.6e-03  3.7e-03  3.6e-03  5.7e-03  7.4e-03     S = 16: 1.1e-02 (512), 1.2e-02 (2048)

and the emulated scan is at 0.98 .. 2.28 times e32 on them (the state: 0.03 .. 1.23), worst at B = 64.
"""
import ctypes

import numpy as np
import pytest

FS = 48000.0
FMIN = 240.0         # see above and test_banks_are_usable
N_BUFFERS = 12
# the scan form's cases of test_eq_gpu.py (the 16 384-track case is measured on its first 64 tracks)
SCAN_SHAPES = [(128, 512), (3, 64), (1000, 128), (7, 1024), (130, 256), (9, 2048)]
SCAN_CASES = [(T, B, S) for (T, B) in SCAN_SHAPES for S in (1, 4, 8, 16)] + [(16384, 512, 8)]


def case_seed(T, B, S):
    return T + B + S


def _rbj_highpass(f, q, fs=FS):
    w0 = 2.0 * np.pi * f / fs
    al = np.sin(w0) / (2.0 * q)
    c = np.cos(w0)
    return np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + al, -2 * c, 1 - al])


def _rbj_peaking(f, q, gain_db, fs=FS):
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * f / fs
    al = np.sin(w0) / (2.0 * q)
    c = np.cos(w0)
    return np.array([1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A])


def _rbj_lowshelf(f, gain_db, fs=FS):
    """Shelf slope 1 (the steepest without overshoot): alpha = sin(w0) / 2 * sqrt(2)."""
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * f / fs
    c = np.cos(w0)
    k = 2.0 * np.sqrt(A) * np.sin(w0) / 2.0 * np.sqrt(2.0)
    return np.array([A * ((A + 1) - (A - 1) * c + k), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - k),
                     (A + 1) + (A - 1) * c + k, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - k])


def eq_bank(T, S, seed, fmin=FMIN):
    """[T][S][5] float32 = {b0,b1,b2,a1,a2}, a0 divided out in float64 and rounded once."""
    rng = np.random.RandomState(seed)
    out = np.empty((T, S, 5), np.float32)
    lo = max(fmin, 60.0)
    for t in range(T):
        for s in range(S):
            if s == 0:
                sec = _rbj_highpass(fmin * 4.0 ** rng.uniform(), np.sqrt(0.5))
            else:
                f = lo * (16000.0 / lo) ** rng.uniform()
                sec = _rbj_peaking(f, 0.5 * 16.0 ** rng.uniform(), rng.uniform(-12.0, 12.0))
            out[t, s] = (sec[[0, 1, 2, 4, 5]] / sec[3]).astype(np.float32)
    return out


def eq_cascade(x, coeffs, state, dtype=np.float32):
    """x [T][B], coeffs [T][S][5], state [T][S][2] = (z1, z2), updated in place.  Vectorised over tracks; every
    operation is one numpy operation in `dtype`, so one rounding each, in the golden's order."""
    T, B = x.shape
    S = coeffs.shape[1]
    assert state.shape == (T, S, 2) and state.dtype == dtype
    y = np.array(x, dtype)
    c = np.asarray(coeffs, dtype)
    for s in range(S):
        b0, b1, b2, a1, a2 = (np.ascontiguousarray(c[:, s, k]) for k in range(5))
        z1, z2 = state[:, s, 0].copy(), state[:, s, 1].copy()
        for i in range(B):
            w = (y[:, i] - a1 * z1) - a2 * z2
            y[:, i] = (b0 * w + b1 * z1) + b2 * z2
            z2 = z1
            z1 = w
        state[:, s, 0], state[:, s, 1] = z1, z2
    assert y.dtype == dtype
    return y


def eq_reference_f32(x, coeffs, state):
    return eq_cascade(np.asarray(x, np.float32), np.asarray(coeffs, np.float32), state, np.float32)


def eq_reference_f64(x, coeffs, zi):
    """sosfilt per track in float64 on the float32 coefficients; zi [T][S][2] is scipy's (transposed-form) state,
    updated in place."""
    signal = pytest.importorskip("scipy.signal")
    T, B = x.shape
    c = np.asarray(coeffs, np.float32).astype(np.float64)
    y = np.empty((T, B), np.float64)
    for t in range(T):
        sos = np.concatenate([c[t, :, :3], np.ones((c.shape[1], 1)), c[t, :, 3:]], axis=1)
        y[t], zi[t] = signal.sosfilt(sos, x[t].astype(np.float64), zi=zi[t])
    return y


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def bank_round_off(T, B, S, seed, coeffs=None, n_buffers=N_BUFFERS, tracks=None, switch=None):
    """(e32 of the outputs, e32 of the DF-II state, y64 per buffer, final float64 DF-II state): what eq_reference_f32
    loses against float64 on this bank and this noise, peak-normalised over the whole run.  tracks: a slice of the job's
    tracks to do it on.  switch = (k, coeffs2): from buffer k on the coefficients are coeffs2, the states kept."""
    coeffs = eq_bank(T, S, seed) if coeffs is None else coeffs
    sl = slice(None) if tracks is None else tracks
    c = coeffs[sl]
    n = c.shape[0]
    st32, st64 = np.zeros((n, S, 2), np.float32), np.zeros((n, S, 2), np.float64)
    zi = np.zeros((n, S, 2), np.float64)
    err = peak = 0.0
    ys = []
    for k in range(n_buffers):
        if switch is not None and k == switch[0]:
            # scipy's transposed-form state belongs to the OLD coefficients: carry the DF-II state over instead
            # (d1 = (b1 - a1 b0) z1 + (b2 - a2 b0) z2, d2 = (b2 - a2 b0) z1 + (b2 a1 - a2 b1) z2 for the new ones)
            c = switch[1][sl]
            b0, b1, b2, a1, a2 = (c[..., i].astype(np.float64) for i in range(5))
            zi[..., 0] = (b1 - a1 * b0) * st64[..., 0] + (b2 - a2 * b0) * st64[..., 1]
            zi[..., 1] = (b2 - a2 * b0) * st64[..., 0] + (b2 * a1 - a2 * b1) * st64[..., 1]
        x = noise(T, B, 1000 * seed + k)[sl]
        y32 = eq_reference_f32(x, c, st32)
        y64 = eq_reference_f64(x, c, zi)
        yc = eq_cascade(x.astype(np.float64), c.astype(np.float64), st64, np.float64)
        # the float64 DF-II recurrence and scipy's transposed form are the same filter
        assert np.abs(yc - y64).max() <= 1e-9 * max(np.abs(y64).max(), 1.0)
        err = max(err, float(np.abs(y32 - y64).max()))
        peak = max(peak, float(np.abs(y64).max()))
        ys.append(y64)
    e_state = float(np.abs(st32 - st64).max() / np.abs(st64).max())
    return err / peak, e_state, ys, st64


# ---- the low band: what a channel strip carries (rumble filter, shelf, hum notch), at 48 and 96 kHz -------------
LOW_T = 24
LOW_CASES = ([(B, S, fs) for B in (64, 128, 256, 512, 1024, 2048) for S in (1, 4) for fs in (48000, 96000)]
             + [(B, 16, fs) for B in (512, 2048) for fs in (48000, 96000)])


def low_seed(B, S, fs):
    return B + S + fs // 48000


def eq_bank_low(T, S, seed, fs):
    """[T][S][5] float32 as eq_bank: section 0 a Q sqrt(1/2) high-pass at 20..80 Hz, section 1 a low shelf at
    60..200 Hz, +-12 dB, the others peaking sections at 20..240 Hz, Q 0.5..30, -24..+12 dB (frequencies and Q
    log-uniform).  Every section is inside the stability triangle after the rounding to float32."""
    assert fs in (48000, 96000)
    rng = np.random.RandomState(seed)
    out = np.empty((T, S, 5), np.float32)
    for t in range(T):
        for s in range(S):
            if s == 0:
                sec = _rbj_highpass(20.0 * 4.0 ** rng.uniform(), np.sqrt(0.5), fs)
            elif s == 1:
                sec = _rbj_lowshelf(60.0 * (200.0 / 60.0) ** rng.uniform(), rng.uniform(-12.0, 12.0), fs)
            else:
                sec = _rbj_peaking(20.0 * 12.0 ** rng.uniform(), 0.5 * 60.0 ** rng.uniform(), rng.uniform(-24.0, 12.0), fs)
            out[t, s] = (sec[[0, 1, 2, 4, 5]] / sec[3]).astype(np.float32)
    a1, a2 = out[..., 3].astype(np.float64), out[..., 4].astype(np.float64)
    assert (np.abs(a2) < 1).all() and (np.abs(a1) < 1 + a2).all()
    return out


_low_cases = {}


def low_case(B, S, fs):
    """(coeffs, e32 of the outputs, e32 of the state, y64 per buffer, final float64 state) of a LOW_CASES entry,
    made once per process and read-only: the host tests and the GPU tests share it."""
    key = (B, S, fs)
    if key not in _low_cases:
        seed = low_seed(B, S, fs)
        coeffs = eq_bank_low(LOW_T, S, seed, fs)
        e_out, e_state, ys, st64 = bank_round_off(LOW_T, B, S, seed, coeffs=coeffs)
        for a in [coeffs, st64] + ys:
            a.flags.writeable = False
        _low_cases[key] = (coeffs, e_out, e_state, tuple(ys), st64)
    return _low_cases[key]


def eq_form(bufsize, sections):
    """(M, H) of the scan a plan runs ("The form"); (0, 0): none."""
    if bufsize < 64 or bufsize > 2048 or bufsize & (bufsize - 1):
        return 0, 0
    m = bufsize // 64
    if m <= 4:
        return m, 1
    M = 4 if sections <= 2 else 8
    return M, m // M


def eq_scan_consts(coeffs, M):
    """(alpha [T][S][M], beta [T][S][M], p [T][S][6][4]) float32: eq_consts_kernel's arithmetic, in float64 on the
    float32 coefficients and rounded once, for the basis (u, d) = (z1, z1 - z2)."""
    c = np.asarray(coeffs, np.float32).astype(np.float64)
    T, S = c.shape[:2]
    A0, A1 = -c[..., 3], -c[..., 4]
    P0, P1, P2, P3 = np.ones((T, S)), np.zeros((T, S)), np.zeros((T, S)), np.ones((T, S))
    alpha, beta = np.empty((T, S, M), np.float32), np.empty((T, S, M), np.float32)
    p = np.empty((T, S, 6, 4), np.float32)
    for i in range(M):
        n0, n1 = A0 * P0 + A1 * P2, A0 * P1 + A1 * P3
        P2, P3, P0, P1 = P0, P1, n0, n1
        alpha[..., i] = P0 + P1
        beta[..., i] = -P1
    for q in range(6):
        p[..., q, 0], p[..., q, 1] = P0 + P1, -P1
        p[..., q, 2], p[..., q, 3] = (P0 + P1) - (P2 + P3), P3 - P1
        P0, P1, P2, P3 = P0 * P0 + P1 * P2, P0 * P1 + P1 * P3, P2 * P0 + P3 * P2, P2 * P1 + P3 * P3
    return alpha, beta, p


def _fmaf(a, b, c):
    """a b + c rounded to float64, then to float32: fmaf but for the double rounding."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _shfl_up(a, d):
    """[T][64]: lane l gets lane l - d; the lanes below d keep their own (and never use it)."""
    out = a.copy()
    out[:, d:] = a[:, :-d]
    return out


def eq_scan_emulated(x, coeffs, state, M, H, consts=eq_scan_consts):
    """eq_scan_kernel<M, H> in numpy float32, vectorised over tracks and lanes: x [T][64 M H], coeffs [T][S][5],
    state [T][S][2] = (z1, z2) float32, updated in place.  Local pass from zero state (lane 0 from the carried
    state), six Kogge-Stone steps on (u, d), homogeneous correction, output taps, in the kernel's operation order.
    Not the device's bits (_fmaf rounds twice) and never a GPU test's expected value: it tells what the ALGORITHM
    loses on a bank, without a GPU."""
    T, B = x.shape
    S = coeffs.shape[1]
    assert B == 64 * M * H and state.shape == (T, S, 2) and state.dtype == np.float32
    c = np.asarray(coeffs, np.float32)
    alpha, beta, p = consts(c, M)
    xs = np.array(x, np.float32).reshape(T, H, 64, M)
    lanes = np.arange(64)
    for s in range(S):
        b0, b1, b2, a1, a2 = (c[:, s, k][:, None] for k in range(5))
        al, be, pw = alpha[:, s], beta[:, s], p[:, s]
        in1, in2 = state[:, s, 0].copy(), state[:, s, 1].copy()
        for h in range(H):
            z1, z2 = np.zeros((T, 64), np.float32), np.zeros((T, 64), np.float32)
            z1[:, 0], z2[:, 0] = in1, in2
            w = np.empty((T, 64, M), np.float32)
            for i in range(M):                                   # 1. local pass
                wv = _fmaf(-a2, z2, _fmaf(-a1, z1, xs[:, h, :, i]))
                z2, z1 = z1, wv
                w[:, :, i] = wv
            e1, e2 = z1, z1 - z2                                 # 2. the scan of the outgoing states
            for q in range(6):
                d = 1 << q
                u1, u2 = _shfl_up(e1, d), _shfl_up(e2, d)
                n1 = _fmaf(pw[:, q, 1, None], u2, _fmaf(pw[:, q, 0, None], u1, e1))
                n2 = _fmaf(pw[:, q, 3, None], u2, _fmaf(pw[:, q, 2, None], u1, e2))
                e1, e2 = np.where(lanes >= d, n1, e1), np.where(lanes >= d, n2, e2)
            s1, s2 = _shfl_up(e1, 1), _shfl_up(e2, 1)
            s1[:, 0] = s2[:, 0] = 0.0
            for i in range(M):                                   # 3. homogeneous correction
                w[:, :, i] = _fmaf(be[:, i, None], s2, _fmaf(al[:, i, None], s1, w[:, :, i]))
            p1 = _shfl_up(w[:, :, M - 1], 1)                     # 4. output taps
            p2 = _shfl_up(w[:, :, M - 2], 1) if M >= 2 else _shfl_up(w[:, :, 0], 2)
            p1[:, 0], p2[:, 0] = in1, in2
            if M == 1:
                p2[:, 1] = in1
            for i in range(M):
                wm1 = w[:, :, i - 1] if i >= 1 else p1
                wm2 = w[:, :, i - 2] if i >= 2 else (p1 if i == 1 else p2)
                xs[:, h, :, i] = _fmaf(b2, wm2, _fmaf(b1, wm1, b0 * w[:, :, i]))
            in1, in2 = w[:, 63, M - 1].copy(), (w[:, 63, M - 2] if M >= 2 else p1[:, 63]).copy()
        state[:, s, 0], state[:, s, 1] = in1, in2
    return xs.reshape(T, B)


def scan_emulation_error(B, S, fs, consts=eq_scan_consts, case=None, T=LOW_T, seed=None):
    """(err of the outputs, err of the state) of eq_scan_emulated against float64, by bank_round_off's yardsticks."""
    coeffs, _, _, ys, st64 = low_case(B, S, fs) if case is None else case
    seed = low_seed(B, S, fs) if seed is None else seed
    M, H = eq_form(B, S)
    st = np.zeros((T, S, 2), np.float32)
    err = peak = 0.0
    for k in range(len(ys)):
        y = eq_scan_emulated(noise(T, B, 1000 * seed + k), coeffs, st, M, H, consts)
        err = max(err, float(np.abs(y - ys[k]).max()))
        peak = max(peak, float(np.abs(ys[k]).max()))
    return err / peak, float(np.abs(st - st64).max() / np.abs(st64).max())


# ---------------------------------------------------------------------------
def test_one_section_reproduces_the_pinned_oracle_bit_for_bit(orc):
    T, B = 37, 300
    for c in (orc.iir_coeffs(0.25), np.array([0.2, 0.1, -0.05, -1.2, 0.72], np.float32)):
        coeffs = np.broadcast_to(np.asarray(c, np.float32), (T, 1, 5)).copy()
        st = np.zeros((T, 1, 2), np.float32)
        st_orc = np.zeros(2 * T, np.float32)
        for k in range(3):
            x = noise(T, B, 50 + k)
            y = eq_reference_f32(x, coeffs, st)
            ref = orc.iir(x.ravel(), c, st_orc, T, B).reshape(T, B)
            assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))
            assert np.array_equal(st.reshape(-1).view(np.uint32), st_orc.view(np.uint32))


def test_sections_compose():
    """Two sections in one call are the first section's output through the second."""
    T, B = 5, 100
    c = eq_bank(T, 2, 3)
    x = noise(T, B, 9)
    st = np.zeros((T, 2, 2), np.float32)
    y = eq_reference_f32(x, c, st)
    sa, sb = np.zeros((T, 1, 2), np.float32), np.zeros((T, 1, 2), np.float32)
    y2 = eq_reference_f32(eq_reference_f32(x, c[:, :1], sa), c[:, 1:], sb)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))
    assert np.array_equal(st[:, 0], sa[:, 0]) and np.array_equal(st[:, 1], sb[:, 0])


def test_banks_are_stable():
    c = eq_bank(256, 16, 11).astype(np.float64)
    a1, a2 = c[..., 3], c[..., 4]
    assert (np.abs(a2) < 1).all() and (np.abs(a1) < 1 + a2).all()


@pytest.mark.parametrize("T,B,S", SCAN_CASES)
def test_banks_are_usable(T, B, S):
    """The yardstick: the bank's own float32 error stays below 1e-4 of peak (else it would test DF-II round-off)."""
    e_out, e_state, _, _ = bank_round_off(T, B, S, case_seed(T, B, S), tracks=slice(0, 64) if T > 1000 else None)
    print("eq_bank(%d, %d, seed %d, fmin=%g) at B = %d: e32 outputs %.3g of peak, state %.3g of peak"
          % (T, S, case_seed(T, B, S), FMIN, B, e_out, e_state))
    assert e_out <= 1e-4, e_out


def test_low_banks_are_stable_and_in_their_band():
    for fs in (48000, 96000):
        c = eq_bank_low(64, 16, 12, fs).astype(np.float64)     # asserts the triangle itself
        b, a1, a2 = c[..., :3], c[..., 3], c[..., 4]
        dc = b.sum(-1) / (1 + a1 + a2)
        assert np.abs(dc[:, 0]).max() < 1e-3                   # the high-pass
        assert (np.abs(20 * np.log10(dc[:, 1])) <= 12.5).all() and np.abs(20 * np.log10(dc[:, 1])).max() > 6
    for g in (-12.0, 5.0):                                     # the shelf: its gain at DC, none at Nyquist
        sec = _rbj_lowshelf(100.0, g, 48000)
        assert abs(20 * np.log10(sec[:3].sum() / sec[3:].sum()) - g) < 1e-9
        assert abs((sec[0] - sec[1] + sec[2]) / (sec[3] - sec[4] + sec[5]) - 1) < 1e-9


def test_the_emulated_scan_is_the_scan_kernels_algorithm():
    """On eq_bank, where the scan's device figures are known (1.2-2.3 times e32), the emulation is an
    equaliser too: within the rule, every form; and with the identity filter it returns its input."""
    for B, S in ((64, 1), (128, 3), (256, 2), (512, 2), (512, 3), (1024, 4), (2048, 1), (2048, 3)):
        T, seed = 6, case_seed(6, B, S)
        coeffs = eq_bank(T, S, seed)
        e_out, e_state, ys, st64 = bank_round_off(T, B, S, seed, coeffs=coeffs, n_buffers=4)
        err, err_state = scan_emulation_error(B, S, None, case=(coeffs, e_out, e_state, ys, st64), T=T, seed=seed)
        assert err <= max(1e-5, 4 * e_out) and err_state <= max(1e-5, 4 * e_state), (B, S, err, e_out, err_state, e_state)
    ident = np.zeros((3, 2, 5), np.float32)
    ident[..., 0] = 1
    x = noise(3, 512, 1)
    assert np.array_equal(eq_scan_emulated(x, ident, np.zeros((3, 2, 2), np.float32), 4, 2), x)


@pytest.mark.parametrize("B,S,fs", LOW_CASES)
def test_low_bank_scan_emulation_is_within_the_rule(B, S, fs):
    """The scan's ALGORITHM (eq_scan_emulated) against float64 on the low bank: within max(1e-5, 4 e32), outputs and
    final state.  That makes the low bank one the device can be held to (test_eq_gpu.py); a failure here is about the
    scan, not about the device."""
    _, e_out, e_state, _, _ = low_case(B, S, fs)
    err, err_state = scan_emulation_error(B, S, fs)
    print("eq scan emulated B=%d S=%d fs=%d form=%s: outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (B, S, fs, eq_form(B, S), err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    assert err <= max(1e-5, 4.0 * e_out), (err, e_out)
    assert err_state <= max(1e-5, 4.0 * e_state), (err_state, e_state)


@pytest.mark.parametrize("B", [64, 128, 256, 512, 1024, 2048])
def test_low_bank_round_off_is_what_it_is(B):
    """The low bank is outside what eq_bank covers: its own float32 round-off exceeds the 1e-4 of peak that
    test_banks_are_usable caps eq_bank at."""
    _, e_out, _, _, _ = low_case(B, 1, 48000)
    assert e_out > 1e-4, e_out


def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    h = ctypes.c_void_p()
    for args in ((-1, 512, 4), (4, 0, 4), (4, 512, 0), (4, 512, 17)):
        assert _capi.lib.gab_eq_create(ctypes.byref(h), *args) == _capi.GAB_ERR_INVALID_ARG, args
        assert b"gab_eq_create" in _capi.lib.gab_last_error()
        assert not h.value
    assert _capi.lib.gab_eq_create(None, 4, 512, 4) == _capi.GAB_ERR_INVALID_ARG
    assert _capi.lib.gab_eq_process(None, None, None, None) == _capi.GAB_ERR_INVALID_ARG
    assert b"null pointer" in _capi.lib.gab_last_error()
    assert _capi.lib.gab_eq_destroy(None) == _capi.GAB_ERR_INVALID_ARG


def test_eq_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "EqPlan" in g.__all__ and callable(g.EqPlan)
    for name in ("set_sos", "set_coeffs", "reset", "process", "process_batch", "state", "form", "close"):
        assert hasattr(g.EqPlan, name), name
