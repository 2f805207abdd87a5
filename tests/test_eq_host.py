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


def _rbj_highpass(f, q):
    w0 = 2.0 * np.pi * f / FS
    al = np.sin(w0) / (2.0 * q)
    c = np.cos(w0)
    return np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + al, -2 * c, 1 - al])


def _rbj_peaking(f, q, gain_db):
    A = 10.0 ** (gain_db / 40.0)
    w0 = 2.0 * np.pi * f / FS
    al = np.sin(w0) / (2.0 * q)
    c = np.cos(w0)
    return np.array([1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A])


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
