"""What every plan says when it refuses a value (gab_last_error), whole and to the letter, and what it keeps.

The texts are written out here, not computed from the library: a caller may match on them.  Every ranged set goes
through the _tracks entry with first_track = 3 and four rows; the offender is in row 1 (so the text says track 4) and a
NaN in row 2 (so the FIRST offender is the one named).  Meter and resample take whole tables.  After its cases a ramped
plan still holds the tables it was given: the old rows in current, the ramped-in rows in target.
"""
import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)

pytestmark = pytest.mark.gpu

T, B = 8, 64
FIRST, ROWS = 3, 4


def refused(gab, call, text):
    with pytest.raises(gab.GabError) as e:
        call()
    assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
    assert gab._capi.lib.gab_last_error().decode() == text


def tables(width, row0, row1):
    """Two admitted tables [T][width] that differ in every row."""
    k = np.arange(T, dtype=np.float32)[:, None]
    a = np.asarray(row0, np.float32)[None, :] * (1.0 - k / 64.0)
    b = np.asarray(row1, np.float32)[None, :] * (1.0 - k / 32.0)
    assert a.shape == (T, width) and b.shape == (T, width)
    return a.astype(np.float32), b.astype(np.float32)


def offending(table, field, value, nan_field=0):
    """Rows FIRST .. FIRST + ROWS of table with `value` at (row 1, field) and a NaN in row 2."""
    rows = table[FIRST:FIRST + ROWS].copy()
    rows[1, field] = value
    rows[2, nan_field] = np.nan
    return dev(rows)


def kept(pair, cur, tgt):
    c, t = pair
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def test_mix(gab):
    p0, p1 = tables(3, [0.5, -0.25, 1.0], [0.125, 2.0, -1.0])
    plan = gab.MixPlan(T, B, 3)
    plan.set_gains(dev(p0), ramp=False)
    plan.set_gains(dev(p1))
    refused(gab, lambda: plan.set_gains(offending(p1, 2, np.inf), first_track=FIRST),
            "gab_mix_set_gains_tracks: the gain of track 4 bus 2 is not finite; the plan keeps its gains")
    assert kept(plan.gains(), p0, p1)
    plan.close()


@pytest.mark.parametrize("field,value,text", [
    (0, 17.0, "track 4 field 0 (delay) must be finite and within [min_delay, max_delay]"),
    (1, 1.0, "track 4 field 1 (feedback) must be finite and below 1 in magnitude"),
    (2, np.inf, "track 4 field 2 (wet) must be finite")])
def test_delay(gab, field, value, text):
    p0, p1 = tables(4, [16.0, 0.5, 1.0, 1.0], [12.0, -0.75, 0.5, 0.25])
    plan = gab.DelayPlan(T, B, 16, "linear")
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    refused(gab, lambda: plan.set_params(offending(p1, field, value, 3), first_track=FIRST),
            "gab_delay_set_params_tracks: " + text + "; the plan keeps its parameters")
    assert kept(plan.params(), p0, p1)
    plan.close()


@pytest.mark.parametrize("field,value,text", [
    (0, 129.0, "track 4 field 0 (thr) must be finite and within [-128, 128]"),
    (1, 0.5, "track 4 field 1 (slope) must be within [-1, 0]"),
    (2, 65.0, "track 4 field 2 (knee) must be within [0, 64]"),
    (3, -1.0, "track 4 field 3 (kq) must be finite and >= 0"),
    (4, 1.0, "track 4 field 4 (att) must be within [0, 1 - 2^-20]"),
    (5, -0.125, "track 4 field 5 (rel) must be within [0, 1 - 2^-20]"),
    (6, np.inf, "track 4 field 6 (makeup) must be finite"),
    (7, 1.0, "track 4 field 7 (range) must be finite and <= 0")])
def test_dynamics(gab, field, value, text):
    p0, p1 = tables(8, [-20.0, -0.5, 6.0, 0.0625, 0.5, 0.75, 1.0, -40.0], [-30.0, -0.75, 12.0, 0.03125, 0.25, 0.875, 2.0, -20.0])
    plan = gab.DynamicsPlan(T, B, link=1)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    refused(gab, lambda: plan.set_params(offending(p1, field, value, 6), first_track=FIRST),
            "gab_dyn_set_params_tracks: " + text + "; the plan keeps its parameters")
    assert kept(plan.params(), p0, p1)
    plan.close()


@pytest.mark.parametrize("field,value,text", [
    (1, 0.5, "track 4 field 1 (g) must be finite and at most gab_reverb_gmax(lines) in magnitude"),
    (6, 1.0, "track 4 field 6 (damp) must be within [0, 1 - 2^-20]"),
    (9, -np.inf, "track 4 field 9 (b) must be finite")])
def test_reverb_parameters(gab, field, value, text):
    # lines 4, outs 1: a row is g[4], damp[4], b[4], c[4], dry
    p0, p1 = tables(17, [0.25] * 4 + [0.5] * 4 + [1.0] * 4 + [0.5] * 4 + [1.0],
                    [-0.375] * 4 + [0.25] * 4 + [0.5] * 4 + [-1.0] * 4 + [0.5])
    plan = gab.ReverbPlan(T, B, lines=4, outs=1, max_delay=64)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    refused(gab, lambda: plan.set_params(offending(p1, field, value, 16), first_track=FIRST),
            "gab_reverb_set_params_tracks: " + text + "; the plan keeps its parameters")
    assert kept(plan.params(), p0, p1)
    plan.close()


def test_reverb_delays(gab):
    d = (32 + (np.arange(T * 4) * 5) % 33).astype(np.int32).reshape(T, 4)
    plan = gab.ReverbPlan(T, B, lines=4, outs=1, max_delay=64)
    plan.set_delays(dev(d))
    rows = d[FIRST:FIRST + ROWS].copy()
    rows[1, 2] = 31             # GAB_REVERB_MIN_DELAY - 1
    rows[2, 0] = 65             # an integer has no NaN: beyond max_delay
    refused(gab, lambda: plan.set_delays(dev(rows), first_track=FIRST),
            "gab_reverb_set_delays_tracks: track 4 line 2 must be within [GAB_REVERB_MIN_DELAY, max_delay]; "
            "the plan keeps its delays")
    assert np.array_equal(host(plan.state()[3]), d)
    plan.close()


def test_eq(gab):
    c = np.tile(np.array([0.5, 0.25, 0.125, -0.5, 0.25], np.float32), (T, 2, 1))
    plan = gab.EqPlan(T, B, 2)
    plan.set_coeffs(dev(c))
    rows = c[FIRST:FIRST + ROWS].copy()
    rows[1, 1, 4] = 1.0         # a2 = 1
    rows[2, 0, 0] = np.nan
    refused(gab, lambda: plan.set_coeffs(dev(rows), FIRST, ROWS),
            "gab_eq_set_coeffs_tracks: track 4 section 1 is unstable (needs |a2| < 1 and |a1| < 1 + a2) or not finite; "
            "the plan keeps its coefficients")
    plan.close()


@pytest.mark.parametrize("where,value,text", [
    ((1, 1), np.nan, "section 1 value 1 (b1)"),
    ((0, 3), 1.5, "section 0 value 3 (a1)")])              # |a1| = 1.5 = 1 + a2
def test_meter(gab, where, value, text):
    sec = np.array([[1.0, -2.0, 1.0, -1.25, 0.5], [0.5, 0.25, 0.125, 0.75, 0.25]], np.float32)
    plan = gab.MeterPlan(T, B, window=1)
    sec[where] = value
    sec[1, 2] = np.nan if where[0] == 0 else sec[1, 2]      # a later offender is not the one named
    refused(gab, lambda: plan.set_weighting(dev(sec)),
            "gab_meter_set_weighting: " + text + " is not finite or outside the stability triangle "
            "(needs |a2| < 1 and |a1| < 1 + a2); the plan keeps its weighting")
    plan.close()


def test_resample(gab):
    plan = gab.ResamplePlan(T, B, 3, 2, taps=8)
    before = host(plan.taps())
    t = before.copy()
    t[2, 5] = np.inf
    t[2, 7] = np.nan
    refused(gab, lambda: plan.set_taps(dev(t)),
            "gab_resample_set_taps: phase 2 tap 5 is not finite; the plan keeps its taps")
    assert np.array_equal(bits(host(plan.taps())), bits(before))
    plan.close()
