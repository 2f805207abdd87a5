"""The saturator plan's restatement (tests/saturator_twin.py) held to known answers that do not trust it, without a GPU:
the curves at their corners, one-hot taps, any cut of a stream against the whole stream, float32 against float64 within
a bound derived here, the closed form on a constant, the two rules, a pinned row of saturator_params, the library's
refusals before any device call, and the point of the plan: less aliasing at R = 4 than at R = 1."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturator_twin as st  # noqa: E402
from saturator_twin import F32, SatTwin  # noqa: E402
from test_resample_host import EPS, Twin as ResampleTwin, noise  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


SUB = F32(2.0 ** -140)           # a subnormal
INF, NAN = F32(np.inf), F32(np.nan)
#            x      hard   cubic      rational
KNOWN = [(0.0,    0.0,   0.0,       0.0),
         (0.5,    0.5,   0.6875,    1.0 / 3.0),      # 0.5 (1.5 - 0.125); 0.5 / 1.5 rounded once
         (1.0,    1.0,   1.0,       0.5),
         (2.0,    1.0,   1.0,       2.0 / 3.0),
         (np.inf, 1.0,   1.0,       np.nan),         # inf / inf
         (float(SUB), float(SUB), 1.5 * float(SUB), float(SUB))]   # 1 + 2^-140 rounds to 1; 1.5 x: 2^-140 + 2^-141, exact


def test_known_answers_of_each_curve():
    for x, hard, cubic, rational in KNOWN:
        for sign in (1.0, -1.0):
            for curve, want in zip(st.CURVES, (hard, cubic, rational)):
                got = st.curve32(F32(sign * x), curve)
                want = F32(sign * F32(want)) if not math.isnan(want) else NAN
                assert got.dtype == F32
                if math.isnan(want):
                    assert np.isnan(got), (x, curve)
                else:
                    assert bits(got) == bits(want), (x, sign, curve, got, want)
    for curve in st.CURVES:
        assert np.isnan(st.curve32(NAN, curve))                          # a NaN passes through every curve
        assert bits(st.curve32(F32(-0.0), curve)) == bits(F32(-0.0))
    assert st.curve32(F32(1.0), "cubic") == F32(1.0) and st.curve32(F32(1e30), "cubic") == F32(1.0)


def test_curves_are_odd_on_bits():
    x = np.concatenate([noise(1, 1, 4000, seed=3).reshape(-1) * F32(3.0), [SUB, F32(1.0), F32(2.0), INF, F32(1e-30)]])
    for curve in st.CURVES:
        a, b = st.curve32(x, curve), st.curve32(-x, curve)
        ok = ~np.isnan(a)
        assert np.array_equal(bits(a[ok]), bits(-b[ok])) and np.array_equal(np.isnan(a), np.isnan(b))
        assert np.allclose(a[ok], st.curve64(x, curve)[ok], rtol=0, atol=4 * EPS)


def test_silence_stays_silence_under_a_bias():
    for curve in st.CURVES:
        twin = SatTwin(2, 16, 2, curve, 4, 4)
        twin.set_params([[3.0, 0.4, 2.0], [0.5, -7.0, 1.0]], ramp=False)
        for _ in range(3):
            assert not twin.process(np.zeros((2, 16), F32)).any()


@pytest.mark.parametrize("R", [2, 4, 8])
def test_one_hot_taps_give_the_curve_delayed_exactly(R):
    """h_p[j0] = 1 in every phase and g[j1] = 1: u[R i + p] = w[i - j0], y[m] = v[m R - j1], so the output is
    level (S(drive w + bias) - S(bias)) of the input j0 + ceil(j1 / R) samples back."""
    Ku, Kd, T, B = 6, 4 * R, 2, 20
    row = np.array([[2.5, 0.25, 0.75], [0.5, -0.5, 3.0]], F32)
    x = noise(5, T, B, seed=R)
    for curve in st.CURVES:
        for j0, j1 in ((0, 0), (2, 1), (5, Kd - 1), (3, R), (1, 2 * R + 1)):
            twin = SatTwin(T, B, R, curve, Ku, Kd)
            up, down = np.zeros((R, Ku), F32), np.zeros(Kd, F32)
            up[:, j0] = 1.0
            down[j1] = 1.0
            twin.set_taps(up, down)
            twin.set_params(row, ramp=False)
            got = np.concatenate([twin.process(b) for b in x], axis=1)
            delay = j0 + -(-j1 // R)
            stream = np.concatenate([np.zeros((T, delay), F32), np.concatenate(list(x), axis=1)], axis=1)[:, :5 * B]
            want = st.shape32(stream, row[:, 0:1], row[:, 1:2], row[:, 2:3], curve)
            assert np.array_equal(bits(got), bits(want)), (curve, j0, j1)


def _whole_stream(x, rows, R, curve, Ku, Kd):
    """x [T][N] and a row per base sample [T][N][3] through twins of ONE buffer of N samples: (y, hist_in, hist_os)."""
    T, N = x.shape
    if R == 1:
        return st.shape32(x, rows[:, :, 0], rows[:, :, 1], rows[:, :, 2], curve), None, None
    up, down = ResampleTwin(T, N, R, 1, K=Ku), ResampleTwin(T, R * N, 1, R, K=Kd)
    u, _ = up.process(x)
    r = np.repeat(rows, R, axis=1)
    y, _ = down.process(st.shape32(u, r[:, :, 0], r[:, :, 1], r[:, :, 2], curve))
    return y, up.hist, down.hist


@pytest.mark.parametrize("R,Ku,Kd,curve", [(1, 0, 0, "cubic"), (2, 6, 8, "hard"), (4, 6, 16, "rational"),
                                           (8, 4, 16, "cubic"), (4, 32, 128, "cubic")])
def test_any_cut_into_buffers_and_batches_equals_the_whole_stream(R, Ku, Kd, curve):
    """Buffers of 1, 5, 64 and 100 (below Ku - 1 and with R B below Kd - 1 among them), a ramp on the first buffer: the
    outputs and both histories are the whole stream's, bit for bit; a batch is its single calls."""
    T = 2
    cur = np.array([[1.0, 0.0, 1.0], [1.0, 0.0, 1.0]], F32)
    tgt = np.array([[4.0, 0.3, 0.5], [0.25, -0.2, 2.0]], F32)
    for B, N in ((1, 96), (5, 200), (64, 448), (100, 700)):
        x = noise(1, T, N, seed=B)[0] * F32(1.5)
        rows = np.concatenate([st.ramped_rows(cur, tgt, B), np.broadcast_to(tgt[:, None, :], (T, N - B, 3))], axis=1)
        want, hin, hos = _whole_stream(x, rows, R, curve, Ku, Kd)
        twin = SatTwin(T, B, R, curve, Ku or None, Kd or None)
        assert (twin.Ku, twin.Kd) == (Ku, Kd)
        twin.set_params(tgt, ramp=True)
        n = N // B
        blocks = x.reshape(T, n, B).transpose(1, 0, 2)
        parts = [twin.process(blocks[0]), twin.process(blocks[1])]          # two single calls, then batches of 3 and the rest
        parts += list(twin.process_batch(blocks[2:5])) + list(twin.process_batch(blocks[5:]))
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(bits(got), bits(want)), (B,)
        if R > 1:
            assert np.array_equal(bits(twin.hist_in), bits(hin)) and np.array_equal(bits(twin.hist_os), bits(hos))
            assert twin.hist_in.shape == (T, Ku - 1) and twin.hist_os.shape == (T, Kd - 1)
        assert not twin.pending and np.array_equal(twin.current, tgt)


def test_apply_takes_a_pending_ramp_as_process_batch_would():
    T, B, R = 2, 8, 2
    a, b = SatTwin(T, B, R, "cubic", 4, 4), SatTwin(T, B, R, "cubic", 4, 4)
    tgt = np.array([[3.0, 0.1, 0.5], [0.5, 0.0, 2.0]], F32)
    u = noise(3, T, R * B, seed=11)
    for t in (a, b):
        t.set_params(tgt, ramp=True)
    whole = a.apply(u)
    parts = np.concatenate([b.apply(u[:1]), b.apply(u[1:])])
    assert np.array_equal(bits(whole), bits(parts)) and not a.pending
    steady = st.shape32(u[1], tgt[:, 0:1], tgt[:, 1:2], tgt[:, 2:3], "cubic")
    assert np.array_equal(bits(whole[1]), bits(steady)) and not np.array_equal(bits(whole[0]), bits(
        st.shape32(u[0], tgt[:, 0:1], tgt[:, 1:2], tgt[:, 2:3], "cubic")))
    assert np.array_equal(bits(whole[0][:, -R:]), bits(st.shape32(u[0], tgt[:, 0:1], tgt[:, 1:2], tgt[:, 2:3],
                                                                  "cubic")[:, -R:]))      # r[B - 1] = 1: the target


def _abs_sums(R, Ku, Kd):
    _, _, hu, hd = st.sat_taps(R, Ku, Kd)
    return float(np.abs(hu.astype(np.float64)).sum(axis=1).max()), float(np.abs(hd.astype(np.float64)).sum())


@pytest.mark.parametrize("R,Ku,Kd", [(2, 32, 64), (4, 32, 128), (8, 32, 256), (4, 6, 16)])
@pytest.mark.parametrize("curve", st.CURVES)
def test_float32_is_within_an_a_priori_bound_of_float64(R, Ku, Kd, curve):
    """With A1 = max_p sum|h_p|, A3 = sum|g|, X the input's peak, L the curve's Lipschitz constant and eps = 2^-24 (half
    an ulp, relative):
      stage 1   Ku roundings, each at most eps of a partial sum that A1 X bounds:            e1 = Ku eps A1 X
      a         |drive| e1 carried, and one rounding of a value below |drive| A1 X + |bias|:  ea = |drive| e1 + eps amax
      S         L ea carried; the curve's own roundings on values of magnitude at most 1.5 (none, three, two): below 4 eps;
                S(bias) the same 4 eps; the difference, at most 2 in magnitude, 2 eps; the product with level one more on
                a value below 2 |level|:                                                     e2 = |level| (L ea + 12 eps)
      stage 3   A3 e2 carried, and Kd roundings on partial sums below A3 V, V = 2 |level|:    e3 = A3 e2 + Kd eps A3 V
    Nothing is measured: the figures come from the tables and the row."""
    T, N = 2, 6 * max(Ku, Kd // R) + 64
    x = noise(1, T, N, seed=R + Ku)[0]
    X = float(np.abs(x).max())
    A1, A3 = _abs_sums(R, Ku, Kd)
    for row in ((1.0, 0.0, 1.0), (8.0, 0.25, 0.5), (0.3, -0.6, 2.0)):
        drive, bias, level = (abs(float(F32(v))) for v in row)
        e1 = Ku * EPS * A1 * X
        ea = drive * e1 + EPS * (drive * A1 * X + bias)
        e2 = level * (st.LIPSCHITZ[curve] * ea + 12 * EPS)
        bound = A3 * e2 + Kd * EPS * A3 * 2.0 * level
        twin = SatTwin(T, N, R, curve, Ku, Kd)
        twin.set_params(np.tile(np.array(row, F32), (T, 1)), ramp=False)
        y32 = twin.process(x).astype(np.float64)
        y64 = st.sat_reference_f64(x, np.array(row, F32), R, curve, Ku, Kd)
        err = float(np.max(np.abs(y32 - y64)))
        print("R=%d (%d, %d) %s %s: float32 - float64 = %.3g, bound %.3g" % (R, Ku, Kd, curve, row, err, bound))
        assert err <= bound
        assert bound < 2e-3 * max(1.0, level)                                    # (a bound that says something)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_constant_input_settles_to_the_closed_form(R):
    """On a constant c phase p of the interpolator settles to c s_p, s_p the sum of row p; the shaped value v_p follows,
    and base output m to sum_j g[j] v_((-j) mod R): the float64 form reaches that within float64's own rounding."""
    c, row = 0.6, np.array([3.0, 0.2, 0.8], F32)
    for curve in st.CURVES:
        if R == 1:
            want = st.shape64(c, *row, curve)
            got = st.sat_reference_f64(np.full((1, 8), c, F32), row, 1, curve)
            assert np.max(np.abs(got - st.shape64(F32(c), *row, curve))) == 0.0 and abs(float(want) - got[0, 0]) < 1e-7
            continue
        Ku, Kd, hu, hd = st.sat_taps(R)
        s = hu.astype(np.float64).sum(axis=1)
        v = st.shape64(float(F32(c)) * s, *row, curve)
        g = hd.astype(np.float64).reshape(-1)
        want = sum(g[j] * v[(-j) % R] for j in range(Kd))
        N = Ku + Kd // R + 40
        got = st.sat_reference_f64(np.full((1, N), c, F32), row, R, curve)[0]
        settled = got[Ku - 1 + -(-(Kd - 1) // R):]
        assert len(settled) >= 40 and np.max(np.abs(settled - want)) <= 1e-13
        assert abs(want - float(st.shape64(float(F32(c)), *row, curve))) < 1e-3     # (and that is the curve of c, nearly)


def test_the_parameter_rule_on_every_spoilt_field():
    for field in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            for track in (0, 2):
                twin = SatTwin(3, 4, 2, "hard", 4, 4)
                table = np.tile(np.array([2.0, 0.1, 0.5], F32), (3, 1))
                table[track, field] = bad
                with pytest.raises(ValueError) as e:
                    twin.set_params(table)
                assert str(e.value) == "track %d field %d (%s) must be finite; the plan keeps its parameters" % (
                    track, field, st.FIELDS[field])
                assert np.array_equal(twin.target, np.tile(np.array(st.NEW_ROW, F32), (3, 1))) and not twin.pending
    twin = SatTwin(3, 4, 2, "hard", 4, 4)
    with pytest.raises(ValueError) as e:
        twin.set_params([[1.0, np.nan, np.inf]], first_track=2)          # the first is named, from first_track on
    assert str(e.value).startswith("track 2 field 1 (bias)")
    twin.set_params([[-3.0, -0.0, 0.0]], first_track=1)                   # any finite value passes, negative ones too
    assert twin.pending and twin.target[1, 0] == -3.0


def test_the_taps_rule_on_every_spoilt_table():
    R, Ku, Kd = 2, 4, 8
    _, _, up, down = st.sat_taps(R, Ku, Kd)
    for bad in (np.nan, np.inf):
        for p, j in ((0, 0), (1, 3)):
            u = up.copy()
            u[p, j] = bad
            assert st.refused_taps(u, down, Ku, Kd) == "up table phase %d tap %d is not finite; the plan keeps its taps" % (p, j)
        d = down.copy()
        d[0, 5] = bad
        assert st.refused_taps(up, d, Ku, Kd) == "down table phase 0 tap 5 is not finite; the plan keeps its taps"
        u = up.copy()
        u[1, 1] = bad
        assert st.refused_taps(u, d, Ku, Kd).startswith("up table phase 1 tap 1")     # the up table is looked at first
    twin = SatTwin(1, 4, R, "hard", Ku, Kd)
    with pytest.raises(ValueError):
        twin.set_taps(up, np.full((1, Kd), np.nan, F32))
    assert np.array_equal(twin.down.taps, down) and st.refused_taps(up, down, Ku, Kd) is None


def test_a_row_of_saturator_params_is_pinned():
    from gpuaudiobench_amd import saturator_params
    row = saturator_params(drive_db=24.0, bias=0.1, level_db=-6.0)
    assert row.dtype == np.float32 and row.shape == (3,)
    assert [float(v).hex() for v in row] == ["0x1.fb2a740000000p+3", "0x1.99999a0000000p-4", "0x1.009b9c0000000p-1"]
    comp = saturator_params(drive_db=24.0, bias=0.1, level_db=-6.0, compensate=True)
    assert comp[2] == F32(10.0 ** (-6.0 / 20.0) / 10.0 ** (24.0 / 20.0)) and comp[0] == row[0]
    table = saturator_params(drive_db=[0.0, 6.0], bias=0.0)
    assert table.shape == (2, 3) and np.array_equal(table[0], np.array(st.NEW_ROW, F32))
    assert np.array_equal(saturator_params(), np.array(st.NEW_ROW, F32))


def test_latency_and_default_taps():
    from gpuaudiobench_amd import SaturatorPlan
    assert SaturatorPlan.CURVES == st.CURVES and SaturatorPlan.FIELDS == st.FIELDS
    assert SaturatorPlan._destroy == "gab_sat_destroy" and hasattr(SaturatorPlan, "prepare")
    for R in (2, 4, 8):
        Ku, Kd, hu, hd = st.sat_taps(R)
        assert (Ku, Kd) == (32, 32 * R) and hu.shape == (R, 32) and hd.shape == (1, 32 * R)
        assert st.latency(R, Ku, Kd) == 32 and st.latency(R, 6, 4 * R) == 5
    assert st.latency(1, 0, 0) == 0


def test_arguments_are_refused_before_any_device_call():
    """Against the built library, without a GPU: every refusal of create with its whole text."""
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()

    def refused(args, text):
        assert lib.gab_sat_create(ctypes.byref(h), *args) == bad
        assert lib.gab_last_error().decode() == "gab_sat_create: " + text and not h.value

    refused((0, 64, 4, 1, 32, 128), "tracks and bufsize must be > 0")
    refused((4, 0, 4, 1, 32, 128), "tracks and bufsize must be > 0")
    refused((4, (1 << 20) + 1, 4, 1, 32, 128), "bufsize must be <= 2^20")
    for R in (0, 3, 16, -2):
        refused((4, 64, R, 1, 32, 128), "oversample must be 1, 2, 4 or 8")
    for curve in (-1, 3):
        refused((4, 64, 4, curve, 32, 128), "curve must be 0 (hard), 1 (cubic) or 2 (rational)")
    for ku, kd in ((4, 0), (0, 8), (32, 32)):
        refused((4, 64, 1, 1, ku, kd), "up_taps and down_taps must be 0 at oversample 1")
    for ku in (0, 2, 5, 66):
        refused((4, 64, 4, 1, ku, 128), "up_taps must be even and 4..64")
    for R, kd in ((4, 0), (4, 4), (4, 12), (4, 264), (2, 6), (8, 8), (8, 24)):
        refused((4, 64, R, 1, 32, kd), "down_taps must be 4..256 and a multiple of 2 * oversample")
    assert lib.gab_sat_create(None, 4, 64, 4, 1, 32, 128) == bad
    assert lib.gab_last_error().decode() == "gab_sat_create: null plan pointer"
    for call, args in (("process", (None, None, None, None)), ("process_batch", (None, None, None, 1, None)),
                       ("apply", (None, None, None, 1, None)), ("set_params", (None, None, 1, None)),
                       ("set_params_tracks", (None, None, 0, 1, 1, None)), ("set_taps", (None, None, None, None)),
                       ("reset", (None, None)), ("info", (None,) * 6), ("params", (None,) * 4), ("state", (None,) * 5),
                       ("destroy", (None,))):
        assert getattr(lib, "gab_sat_" + call)(*args) == bad
        assert lib.gab_last_error().decode() == "gab_sat_%s: null pointer" % call


def _aliased_power_db(y, k0, N):
    """The power outside the fundamental (bin k0) and DC of the last N samples under a 4-term Blackman-Harris window,
    over the fundamental's, in dB.  A sine above a quarter of the rate has every harmonic above Nyquist: whatever lies
    outside the fundamental's lobe has folded back."""
    n = np.arange(N)
    w = 0.35875 - 0.48829 * np.cos(2 * np.pi * n / N) + 0.14128 * np.cos(4 * np.pi * n / N) - \
        0.01168 * np.cos(6 * np.pi * n / N)
    P = np.abs(np.fft.rfft(y[-N:] * w)) ** 2
    keep = np.ones(len(P), bool)
    keep[:8] = False
    keep[k0 - 8:k0 + 9] = False
    return 10.0 * np.log10(P[keep].sum() / P[k0 - 8:k0 + 9].sum())


def test_oversampling_by_four_lowers_the_aliased_power():
    """The point of the plan, a property of the design formula and not of the kernel: a sine at 1229 / 4096 = 0.30005 of
    the rate, 24 dB into the hard curve, through the float64 form with the default taps.
    Measured here: aliased power over the fundamental's -7.29 dB at R = 1 and -22.71 dB at R = 4, 15.41 dB lower (the
    third harmonic, at 1/3 of the fundamental, folds to 0.1 of the rate at R = 1; at R = 4 the first component to fold
    into the band is the thirteenth).  Asserted with 3 dB of margin taken off: at least 12.41 dB."""
    N, k0 = 4096, 1229
    x = np.sin(2 * np.pi * k0 / N * np.arange(N + 512)).astype(F32)[None, :]
    row = np.array([10.0 ** (24.0 / 20.0), 0.0, 1.0], F32)
    a1 = _aliased_power_db(st.sat_reference_f64(x, row, 1, "hard")[0], k0, N)
    a4 = _aliased_power_db(st.sat_reference_f64(x, row, 4, "hard")[0], k0, N)
    print("aliased power over the fundamental: R = 1 %.2f dB, R = 4 %.2f dB, difference %.2f dB" % (a1, a4, a1 - a4))
    assert a1 - a4 >= 12.41
