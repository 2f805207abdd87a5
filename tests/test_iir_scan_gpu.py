"""gab_iir's wave scan (iir_scan_kernel) on the device, held to float64 on audio-band sections.

The bank, the rule and the references are test_iir_scan_host.py's: every IIR_BANK entry in every (M, H) form gab_iir
launches, outputs and carried state within max(1e-5, 4 e32) of the float64 peak, where float64 is scipy's sosfilt on
the float32 coefficients and e32 is what the ordered float32 form (eq_reference_f32) loses against it on the same
input, computed here.  Nothing here compares with iir_scan_emulated: the host file has shown that the scan's
arithmetic passes the rule on this bank, so a failure here is the device code's.  Every case prints err / e32
(pytest -s).
"""
import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_eq_host import N_BUFFERS, eq_cascade, eq_reference_f32, noise
from test_iir_scan_host import BANK, BANK_NAMES, C2, REFERENCE, iir_form, iir_reference, is_stable, rule, scan_errors

pytestmark = pytest.mark.gpu

# every (M, H) gab_iir has; 5 tracks leave a partly filled last workgroup, 16 387 one in the segmented form
SHAPES = [(12, 64), (5, 128), (12, 256), (12, 512), (12, 1024), (16384, 512), (16387, 1024)]
FORM_OF = {(12, 64): (1, 1), (5, 128): (2, 1), (12, 256): (4, 1), (12, 512): (8, 1), (12, 1024): (16, 1),
           (16384, 512): (4, 2), (16387, 1024): (4, 4)}


def twins(T):
    """Rows that carry a copy of track 0's input: another wave of its workgroup, the middle, the last track."""
    return [1, T // 2, T - 1]


def checked_rows(T):
    """The tracks held against float64: all of a small job; of 16 384 and more the first 4, 4 around T / 2 and the
    last 4 (the filter is shared, so the reference needs only those rows of the noise)."""
    return np.arange(T) if T < 16384 else np.r_[0:4, T // 2 - 2:T // 2 + 2, T - 4:T]


_inputs = {}


def shape_inputs(T, B):
    """(device buffers [n] of T * B, their checked rows on the host [n][rows][B]): uniform noise, track 0's input
    repeated in twins(T); 12 buffers, 4 from 16 384 tracks on.  Shared by the bank's entries; one large shape at a
    time is kept."""
    if (T, B) not in _inputs:
        for key in [k for k in _inputs if k[0] >= 16384]:
            del _inputs[key]
        rows = checked_rows(T)
        xd, xr = [], []
        for k in range(N_BUFFERS if T < 16384 else 4):
            x = noise(T, B, 1000 * (T + B) + k)
            x[twins(T)] = x[0]
            xd.append(dev(x.ravel()))
            xr.append(x[rows].copy())
        _inputs[(T, B)] = (xd, xr)
    return _inputs[(T, B)]


def run_iir(gab, xd, c, T, B, rows, sequential=False):
    """The buffers xd through gab.iir on one carried state: (outputs of `rows` per buffer, final state [T][2]);
    asserts on the way that every output is finite and that the twins of track 0 have its bits."""
    import torch
    st = dev(np.zeros(2 * T, np.float32))
    idx, tw = dev(np.asarray(rows, np.int64)), dev(np.asarray(twins(T), np.int64))
    ys = []
    for k, x in enumerate(xd):
        y = gab.iir(x, c, st, T, B, sequential=sequential).view(T, B)
        assert bool(torch.isfinite(y).all()), k
        assert bool((y[tw].view(torch.int32) == y[0].view(torch.int32)).all()), "buffer %d: a twin of track 0 differs" % k
        ys.append(host(y[idx]))
    state = host(st).reshape(T, 2)
    assert np.array_equal(bits(state[twins(T)]), bits(np.broadcast_to(state[0], (3, 2)))), "a twin's state differs"
    return ys, state


# ---- 1. the rule, every bank entry in every form -------------------------------------------------------------------
@pytest.mark.parametrize("name", BANK_NAMES)
@pytest.mark.parametrize("T,B", SHAPES)
def test_scan_within_the_rule(gab, T, B, name):
    assert iir_form(T, B) == FORM_OF[(T, B)]
    c = BANK[name]
    rows = checked_rows(T)
    xd, xr = shape_inputs(T, B)
    ref = iir_reference(c, xr)
    e_out, e_state = ref[:2]
    ys, state = run_iir(gab, xd, c, T, B, rows)
    err, err_state = scan_errors(ys, state[rows], ref)
    print("iir scan %s T=%d B=%d form=%s: outputs %.3g of peak (e32 %.3g, ratio %.2f), state %.3g (e32 %.3g, ratio %.2f)"
          % (name, T, B, FORM_OF[(T, B)], err, e_out, err / e_out, err_state, e_state, err_state / e_state))
    assert err <= rule(e_out), (err, e_out)
    assert err_state <= rule(e_state), (err_state, e_state)


@pytest.mark.parametrize("T,B", SHAPES)
def test_scan_keeps_the_reference_filter(gab, orc, T, B):
    """The bar the suite always had (test_iir_wave_scan_with_carried_state), on the two filters it always used: within
    1e-5 of the float32 golden's peak, outputs and carried state."""
    for c in (REFERENCE, C2):
        st_ref = np.zeros(2 * T, np.float32)
        st = dev(np.zeros(2 * T, np.float32))
        for k in range(3):
            x = noise(T, B, 7 * (T + B) + k).ravel()
            y = host(gab.iir(dev(x), c, st, T, B))
            ry = orc.iir(x, c, st_ref, T, B)
            assert np.abs(y - ry).max() <= 1e-5 * np.abs(ry).max(), (c, k)
            assert np.abs(host(st) - st_ref).max() <= 1e-5 * np.abs(st_ref).max(), (c, k)


# ---- 2. a check that shares no recursion with the references -------------------------------------------------------
@pytest.mark.parametrize("name", ["hp30", "bell50_q30"])
def test_settled_sine_gain(gab, name):
    """A 50 Hz sine of amplitude 0.5 (12 tracks, 12 phases) through 40 buffers of 512: the amplitude of the last
    buffer, by least squares on sin and cos, is 0.5 |H(e^jw)|, H evaluated in float64 from the float32 coefficients.
    The bound is four times what the ordered float32 form (eq_reference_f32) misses that by on the same input,
    computed here; the float64 recurrence itself misses it by less than 1e-3 of that bound, so the settling and the
    fit contribute nothing.  The high-pass starts from zero state: its transient falls to e^-57 in 40 buffers.  The
    bell's poles have radius 0.99992, its transient would still be at 0.2 and any bound taken from the float32 form
    would be vacuous: it starts from the sine's steady state (w = x / A(z) in float64, rounded to float32, the same
    for the device and for the float32 form), so that the amplitude is |H| from the first sample."""
    fs, f, T, B, n_buf, amp = 48000.0, 50.0, 12, 512, 40, 0.5
    c32 = BANK[name]
    c = c32.astype(np.float64)
    assert iir_form(T, B) == (8, 1)
    w = 2.0 * np.pi * f / fs
    z = np.exp(-1j * w)
    A = 1 + c[3] * z + c[4] * z * z
    gain = abs((c[0] + c[1] * z + c[2] * z * z) / A)
    phase = 2.0 * np.pi * np.arange(T) / T
    n = np.arange(n_buf * B)
    x = (amp * np.sin(w * n[None, :] + phase[:, None])).astype(np.float32)
    radius = float(np.abs(np.roots([1.0, c[3], c[4]])).max())
    start = np.zeros((T, 1, 2))
    if radius ** (n_buf * B) > 1e-7:            # the steady state: w[n] = Im(amp e^(j (w n + phase)) / A(e^jw)) at n = -1, -2
        for i, m in enumerate((-1, -2)):
            start[:, 0, i] = (amp * np.exp(1j * (w * m + phase)) / A).imag
    start32 = start.astype(np.float32)

    def miss(y_last):
        """relative miss of the fitted amplitude of the last buffer, worst track"""
        nn = n[-B:]
        D = np.stack([np.sin(w * nn), np.cos(w * nn)], axis=1)
        coef = np.linalg.lstsq(D, np.asarray(y_last, np.float64).T, rcond=None)[0]
        return float(np.abs(np.hypot(coef[0], coef[1]) / (amp * gain) - 1).max())

    coeffs = np.broadcast_to(c32, (T, 1, 5)).copy()
    st32, st64 = start32.copy(), start32.astype(np.float64)
    y32 = eq_reference_f32(x, coeffs, st32)[:, -B:]
    y64 = eq_cascade(x.astype(np.float64), coeffs.astype(np.float64), st64, np.float64)[:, -B:]
    miss32, miss64 = miss(y32), miss(y64)
    st = dev(start32.reshape(-1))
    for k in range(n_buf):
        y = gab.iir(dev(x[:, k * B:(k + 1) * B].ravel()), c32, st, T, B)
    got = miss(host(y).reshape(T, B))
    print("iir settled sine %s: |H| = %.6g, relative miss of the amplitude: scan %.3g, ordered float32 %.3g (ratio %.2f), float64 %.3g"
          % (name, gain, got, miss32, got / miss32, miss64))
    assert miss64 <= 1e-3 * 4.0 * miss32, (miss64, miss32)
    assert got <= 4.0 * miss32, (got, miss32)


# ---- 3. tracks do not leak, shapes and sections the scan cannot take -----------------------------------------------
@pytest.mark.parametrize("name,B", [("hp30", 128), ("hp30", 1024), ("bell50_q30", 64), ("bell50_q30", 512),
                                    ("hp30_mirror", 256)])
def test_a_nan_or_infinity_stays_in_its_track(gab, name, B):
    """A NaN in track 3 and an infinity in track 7 of 12, in buffer 1 of 3: every other track has the bits of the run
    without them, outputs and state; the two tracks are not finite from that sample on."""
    T, at = 12, 37
    c = BANK[name]
    hit = np.array([3, 7])
    others = np.setdiff1d(np.arange(T), hit)
    sc, sd = dev(np.zeros(2 * T, np.float32)), dev(np.zeros(2 * T, np.float32))
    for k in range(3):
        x = noise(T, B, 900 + k)
        yc = host(gab.iir(dev(x.ravel()), c, sc, T, B)).reshape(T, B)
        if k == 1:
            x[3, at], x[7, at] = np.nan, np.inf
        yd = host(gab.iir(dev(x.ravel()), c, sd, T, B)).reshape(T, B)
        assert np.array_equal(bits(yd[others]), bits(yc[others])), k
        if k == 0:
            assert np.array_equal(bits(yd), bits(yc))
        elif k == 1:
            assert np.isfinite(yd[hit, :at]).all() and not np.isfinite(yd[hit, at:]).any()
        else:
            assert not np.isfinite(yd[hit]).any()
    sc, sd = host(sc).reshape(T, 2), host(sd).reshape(T, 2)
    assert np.array_equal(bits(sd[others]), bits(sc[others]))
    assert np.isfinite(sc).all() and not np.isfinite(sd[hit]).any()


def _both_forms(gab, x_of, c, T, B, n_buffers=3):
    """n_buffers through gab.iir and through gab.iir(sequential=True), each on its own carried state:
    ([outputs], state) of both.  x_of(k): the k-th device buffer (made once per call, so both get the same)."""
    res = []
    for sequential in (False, True):
        st = dev(np.zeros(2 * T, np.float32))
        ys = [host(gab.iir(x_of(k), c, st, T, B, sequential=sequential)) for k in range(n_buffers)]
        res.append((ys, host(st)))
    return res


def test_shapes_without_a_scan_are_the_ordered_form(gab):
    """A buffer size the scan does not have, and a view that starts 4 bytes in: gab_iir_sequential's bits, outputs and
    state, on the 30 Hz high-pass (where the scan's bits differ from the ordered form's at once)."""
    import torch
    c = BANK["hp30"]
    for T, B in ((12, 100), (5, 2048)):
        assert iir_form(T, B) == (0, 0)
        xs = [dev(noise(T, B, 40 + k).ravel()) for k in range(3)]
        (ys, st), (yq, sq) = _both_forms(gab, lambda k: xs[k], c, T, B)
        for k in range(3):
            assert np.array_equal(bits(ys[k]), bits(yq[k])), (T, B, k)
        assert np.array_equal(bits(st), bits(sq)), (T, B)
    T, B = 12, 512
    assert iir_form(T, B) == (8, 1)
    bufs = []
    for k in range(3):
        buf = torch.zeros(T * B + 1, device="cuda")
        buf[1:] = dev(noise(T, B, 50 + k).ravel())
        assert buf[1:].data_ptr() % 16 == 4
        bufs.append(buf)
    (ys, st), (yq, sq) = _both_forms(gab, lambda k: bufs[k][1:], c, T, B)
    for k in range(3):
        assert np.array_equal(bits(ys[k]), bits(yq[k])), k
    assert np.array_equal(bits(st), bits(sq))
    # and the aligned call does take the scan (the ordered form would pass every rule above): other bits
    y_scan = host(gab.iir(bufs[0][1:].clone(), c, dev(np.zeros(2 * T, np.float32)), T, B))
    assert not np.array_equal(bits(y_scan), bits(ys[0]))


@pytest.mark.parametrize("T,B,c", [(12, 512, [0.5, 0.2, 0.1, -0.3, 1.01]), (12, 64, [0.5, 0.2, 0.1, np.nan, 0.5])])
def test_unstable_or_non_finite_coefficients_take_the_ordered_form(gab, orc, T, B, c):
    """A section outside the stability triangle, or with a value that is not finite, has no scan constants worth the
    name (its powers overflow, inf * 0 is NaN where the golden has a number): gab_iir gives what gab_iir_sequential
    and the golden give -- the same NaN mask, the same bits elsewhere, the same state."""
    c = np.array(c, np.float32)
    assert not is_stable(c) and iir_form(T, B) != (0, 0)
    xs = [noise(T, B, 60 + k).ravel() for k in range(3)]
    xd = [dev(x) for x in xs]
    (ys, st), (yq, sq) = _both_forms(gab, lambda k: xd[k], c, T, B)
    st_ref = np.zeros(2 * T, np.float32)
    refs = [orc.iir(x, c, st_ref, T, B) for x in xs]

    def same(a, b):
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])

    for k in range(3):
        assert same(ys[k], yq[k]) and same(ys[k], refs[k]), k
    assert same(st, sq) and same(st, st_ref)
    if np.isfinite(c).all():
        assert np.isfinite(refs[-1]).all() and np.abs(refs[-1]).max() > 10 * np.abs(refs[0]).max()      # it does grow
    else:
        assert np.isnan(refs[0]).any()
