"""The limiter plan (gab_lim_*) without a GPU: tests/limiter_twin.py, the restatement the GPU tests compare against, held
without trusting it: known answers in dyadic values, the guarantee with <=, the doubling forms against brute force, the
release's decay, cuts of a stream, float32 against float64, linking, samples that are not finite, ramps, the rule.

The a-priori bound of |g32 - g64| (lim_bound), u = 2^-24, for ceilings and detector values in the normal range:
  * xd = drive x: one product, relative u, so the detector is off by a factor within 1 +- u.
  * the need t = ceil / d <= 1: the detector's u, the quotient's rounding u, and the one-unit correction, at most 2^-23 of t
    = 2 u.  A branch taken differently by the two (d <= ceil) happens only where ceil / d is within those of 1 and costs
    nothing beyond them.                                                                                        dt = 4 u
  * the window minimum passes errors unchanged (fminf is 1-Lipschitz in every operand).
  * the release e' = fminf(m, (1 - rel) e + rel): the second operand contracts an error of e by (1 - rel), the fminf
    passes the larger of its operands' errors.  Each step adds its own two roundings, of 1 - e (at most u / 2: the result
    is at most 1) and of the fmaf (at most u / 2), which the recurrence keeps within u / rel; with rel = 0 the step is
    fminf(m, e), exact.                                                              de = dt + (rel > 0 ? u / rel : 0)
  * the box: level h adds two sums of h terms <= 1 each, a rounding of at most u 2h; a result holds W / 2h such additions
    of level h, W u per level, k W u in all, k u after the exact scaling by 2^-k.                          ds = de + k u
  * g = fminf(s, t[n - (W-1)]) passes the larger.                                                             dg = ds
Derived, not measured; second-order terms are covered by a factor 1 + 2^-20.  The figures of every case: pytest -s.

Without the feature every test here fails at the import of limiter_params.
"""
import ctypes

import numpy as np
import pytest

from gpuaudiobench_amd import limiter_params
from limiter_twin import (CEIL, DRIVE, FIELDS, IDENTITY, REL, Twin, first_refused, lim_mix, lim_reference, need_f32,
                          row, sample_params, table, window_min, window_sum)
from plan_helpers import bits
from test_mix_host import mix_ramp

f32 = np.float32
U = 2.0 ** -24
CEILINGS = (1.0, 0.891, 0.999999, 1.2345, 0.5)


def lim_bound(k, rel):
    return (4.0 + k + (1.0 / rel if rel > 0.0 else 0.0)) * U * (1.0 + 2.0 ** -20)


def hot_noise(T, N, seed, ceilings):
    """Noise with peaks 50 x the ceiling of its track."""
    x = np.random.RandomState(seed).uniform(-1.0, 1.0, (T, N))
    return (x * 50.0 * np.asarray(ceilings, np.float64)[:, None]).astype(np.float32)


def run(twin, x, cuts=None):
    """The stream x [T][N] through the twin in buffers of the lengths `cuts` (None: at once): (y, gr per buffer, g)."""
    ys, grs, gs, at = [], [], [], 0
    for n in (cuts or [x.shape[1]]):
        y, gr = twin.process(x[:, at:at + n])
        ys.append(y), grs.append(gr), gs.append(twin.g)
        at += n
    assert at == x.shape[1]
    return np.concatenate(ys, axis=1), np.stack(grs), np.concatenate(gs, axis=1)


def steady(T, W, link=1, wide=False, **kw):
    twin = Twin(T, 1, W, link, wide)
    twin.set_params(table(T, **kw), ramp=False)
    return twin


# ---- known answers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [0.0, 1.0])
def test_one_impulse_in_dyadic_values(rel):
    W, q, N = 8, 20, 60
    x = np.zeros((1, N), np.float32)
    x[0, q] = 4.0
    twin = steady(1, W, ceil=1.0, rel=rel)
    y, gr, g = run(twin, x)
    assert (g[0, :q] == 1.0).all()
    i = np.arange(W)
    assert np.array_equal(g[0, q:q + W], ((W - 1 - i + (i + 1) / 4.0) / W).astype(np.float32))   # exact: dyadic
    assert y[0, q + W - 1] == 1.0 and np.count_nonzero(y) == 1
    if rel == 0.0:
        assert (g[0, q + W:] == 0.25).all() and gr[0, 0] == 0.25
    else:                                                             # the mirror image: the 0.25s leave the box one by one
        i = np.arange(1, W + 1)
        assert np.array_equal(g[0, q + W - 1 + i], ((W - i) / 4.0 + i) / W)
        assert (g[0, q + 2 * W - 1:] == 1.0).all()


# ---- the guarantee ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 9))
def test_the_ceiling_holds_on_every_sample(k):
    W, N = 1 << k, 4096
    rels = (0.0, 0.01, 0.3, 1.0)
    ceil = np.repeat(np.array(CEILINGS, np.float64).astype(np.float32), len(rels))
    T = len(ceil)
    p = table(T)
    p[:, CEIL], p[:, REL] = ceil, np.tile(rels, len(CEILINGS))
    twin = Twin(T, N, W)
    twin.set_params(p, ramp=False)
    y, gr, g = run(twin, hot_noise(T, N, 10 + k, ceil))
    assert (np.abs(y) <= ceil[:, None]).all()                          # <=, float32 against float32
    assert (gr[0] < 0.1).all() and (g >= 0.0).all() and twin.over > T * N // 2
    print("k = %d: largest |y| / ceil %.9f, %d of %d samples over, the correction fired on %d"
          % (k, float((np.abs(y).astype(np.float64) / ceil[:, None]).max()), twin.over, T * N, twin.fired))


def test_census_of_the_correction():
    """Where the quotient's product lands above the ceiling: often at 0.891 and 0.999999, never at 1 and 0.5 (a power of
    two as the numerator: fl(c / d) d rounds to c or below)."""
    N = 1 << 16
    for c in CEILINGS:
        c32 = f32(c)
        d = np.abs(hot_noise(1, N, 99, [c]))
        t, over, fired = need_f32(d, np.full_like(d, c32))
        share = fired.sum() / over.sum()
        print("ceil %-9g: %d over, the correction fired on %.1f %%" % (c, over.sum(), 100.0 * share))
        assert over.sum() > N // 2
        assert (t * d <= c32).all() and (t[over] > 0).all()
        if c in (0.891, 0.999999):
            assert share > 0.05
        if c in (1.0, 0.5):
            assert fired.sum() == 0


# ---- linearity ---------------------------------------------------------------------------------------------------
def test_below_the_ceiling_the_plan_is_a_delay():
    for W in (4, 64, 256):
        D, T, N = W - 1, 3, 700
        x = np.random.RandomState(W).uniform(-1.0, 1.0, (T, N)).astype(np.float32)
        twin = steady(T, W, drive=0.75, ceil=0.75, rel=0.01)
        y, gr, g = run(twin, x, [300, 400])
        want = np.concatenate([np.zeros((T, D), np.float32), f32(0.75) * x[:, :N - D]], axis=1)
        assert np.array_equal(bits(y), bits(want)) and (gr == 1.0).all() and (g == 1.0).all()


def test_a_new_plans_row_is_a_pure_delay():
    W, T, N = 16, 2, 100
    twin = Twin(T, N, W)
    assert np.array_equal(twin.cur, np.tile(IDENTITY, (T, 1))) and first_refused(twin.cur) is None
    x = (np.random.RandomState(1).uniform(-1.0, 1.0, (T, N)) * 2.0 ** 31).astype(np.float32)
    x[0, 5], x[1, 7], x[1, 9] = np.inf, np.nan, -0.0
    y, gr = twin.process(x)
    want = np.concatenate([np.zeros((T, W - 1), np.float32), x[:, :N - (W - 1)]], axis=1)
    both = np.isnan(y) & np.isnan(want)
    assert np.array_equal(np.where(both, 0, bits(y)), np.where(both, 0, bits(want))) and (gr == 1.0).all()


# ---- the doubling forms ------------------------------------------------------------------------------------------
def test_doubling_minimum_is_the_brute_force_minimum():
    rng = np.random.RandomState(3)
    for W in (4, 8, 32, 256):
        tt = rng.uniform(0.0, 1.0, (2, W - 1 + 300)).astype(np.float32)
        brute = np.stack([tt[:, n:n + W].min(axis=1) for n in range(300)], axis=1)
        assert np.array_equal(window_min(tt, W), brute)


def test_doubling_sum_is_the_tree_as_written():
    def tree(e, n, h):                                                # S_h[n], float32 scalars
        return e[n] if h == 1 else f32(tree(e, n, h // 2) + tree(e, n - h // 2, h // 2))

    rng = np.random.RandomState(4)
    for W in (4, 16, 128):
        ee = rng.uniform(0.0, 1.0, (1, W - 1 + 40)).astype(np.float32)
        got = window_sum(ee, W)
        for n in range(40):
            assert got[0, n] == tree(ee[0], n + W - 1, W), (W, n)
        assert not np.array_equal(got, np.stack([ee[:, n:n + W].sum(axis=1) for n in range(40)], axis=1)) or W == 4


# ---- the release -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [0.5, 0.01, 0.001])
def test_the_release_decays_geometrically(rel):
    """Behind a peak 1 - e follows (1 - t)(1 - rel)^n.  Each step rounds 1 - e and the fmaf, at most 2^-25 each, and the
    step contracts: after n steps e is within n 2^-24 of the real recursion on the float32 rel."""
    W, q, N = 4, 5, 400
    x = np.zeros((1, N), np.float32)
    x[0, q] = 3.0
    twin = steady(1, W, ceil=1.0, rel=rel)
    es = []
    for n in range(N):
        twin.process(x[:, n:n + 1])
        es.append(float(twin.hist[2][0, -1]))
    t = float(f32(1.0) / f32(3.0))
    last = q + W - 1                                                  # the last sample whose window holds the peak
    assert es[q] == es[last] == t or abs(es[last] - t) <= 2.0 ** -24
    r = float(f32(rel))
    worst = 0.0
    for n in range(1, N - last):
        want = 1.0 - (1.0 - es[last]) * (1.0 - r) ** n
        worst = max(worst, abs(es[last + n] - want) / (n * U))
        assert abs(es[last + n] - want) <= n * U, n
    print("rel %g: worst error / (n 2^-24) = %.3f" % (rel, worst))


# ---- cuts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8, 64, 128, 256])
def test_any_cut_into_buffers_is_the_whole_stream(W):
    T = 4
    cuts = [1, 3, W - 2, W - 1, W, 64, 65, 200]
    np.random.RandomState(W).shuffle(cuts)
    N = sum(cuts)
    p = lim_mix(T, 2)
    x = hot_noise(T, N, 5, p[:, CEIL] / 10.0)
    whole, parts = Twin(T, N, W, 2), Twin(T, N, W, 2)
    for t in (whole, parts):
        t.set_params(p, ramp=False)
    y0, gr0, g0 = run(whole, x)
    y1, gr1, g1 = run(parts, x, cuts)
    assert np.array_equal(bits(y0), bits(y1)) and np.array_equal(bits(g0), bits(g1))
    assert np.array_equal(gr0[0], gr1.min(axis=0))
    for a, b in zip(whole.hist, parts.hist):
        assert a.shape == (T, W - 1) and np.array_equal(bits(a), bits(b))
    assert (g0 < 1.0).any()


# ---- float32 against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("k", [2, 5, 8])
def test_float32_gain_is_within_its_bound_of_float64(k, rel):
    W, N = 1 << k, 2048
    ceil = np.array(CEILINGS, np.float64).astype(np.float32)
    T = len(ceil)
    p = table(T, rel=rel)
    p[:, CEIL] = ceil
    x = hot_noise(T, N, 10 + k, ceil)
    g = []
    for wide in (False, True):
        twin = Twin(T, N, W, 1, wide)
        twin.set_params(p, ramp=False)
        g.append(run(twin, x)[2].astype(np.float64))
    worst, bound = float(np.abs(g[0] - g[1]).max()), lim_bound(k, float(f32(rel)))
    print("k = %d, rel %g: |g32 - g64| %.3g, bound %.3g (err / bound %.3g)" % (k, rel, worst, bound, worst / bound))
    assert bound <= 2.0 ** -18                                         # the bound itself means something: 3e-5 dB
    assert worst <= bound


# ---- linking -----------------------------------------------------------------------------------------------------
def test_linked_tracks_with_equal_rows_have_equal_gains():
    W, T, N = 16, 4, 500
    x = hot_noise(T, N, 8, [0.05, 0.02, 0.03, 0.001])
    gains = {}
    for link in (1, 2, 4):
        twin = steady(T, W, link, ceil=0.5, rel=0.05)
        gains[link] = run(twin, x)[2]
    assert np.array_equal(gains[2][0], gains[2][1]) and np.array_equal(gains[2][2], gains[2][3])
    assert not np.array_equal(gains[2][0], gains[2][2])
    assert all(np.array_equal(gains[4][0], gains[4][j]) for j in range(1, 4))
    assert not np.array_equal(gains[1][0], gains[1][1])
    assert (gains[2][1] <= gains[1][1]).all()                          # the quieter track follows the louder one down


# ---- samples that are not finite ---------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [1, 2])
def test_nonfinite_samples_reach_one_output_sample_and_nothing_else(link):
    W, T, B = 8, 2, 40
    D, q = W - 1, 36                                                  # D samples from the first buffer's end: it is in the history
    x = hot_noise(T, 2 * B, 6, [0.05, 0.05])
    x0 = x.copy()
    x[0, q], x[1, q + 2] = np.nan, -np.inf
    x0[0, q] = x0[1, q + 2] = 0.0
    a, b = steady(T, W, link, ceil=0.5, rel=0.1), steady(T, W, link, ceil=0.5, rel=0.1)
    for k in range(2):
        (y, gr), (y0, gr0) = a.process(x[:, k * B:(k + 1) * B]), b.process(x0[:, k * B:(k + 1) * B])
        differ = bits(y) != bits(y0)
        assert np.array_equal(gr, gr0) and np.isfinite(a.g).all() and np.array_equal(bits(a.g), bits(b.g))
        if k == 0:
            assert not differ.any()
            hx = bits(a.hist[0]) != bits(b.hist[0])
            assert hx.sum() == 2 and hx[0, D - (B - q)] and hx[1, D - (B - q - 2)]
        else:
            assert differ.sum() == 2 and np.isnan(y[0, q + D - B]) and differ[1, q + 2 + D - B]
            assert np.isinf(y[1, q + 2 + D - B]) or np.isnan(y[1, q + 2 + D - B])
            assert np.array_equal(bits(a.hist[0]), bits(b.hist[0]))
        assert np.array_equal(bits(a.hist[1]), bits(b.hist[1])) and np.array_equal(bits(a.hist[2]), bits(b.hist[2]))


# ---- ramps -------------------------------------------------------------------------------------------------------
def test_the_guarantee_holds_against_a_ramped_ceiling():
    W, T, B = 32, 6, 200
    D = W - 1
    p0, p1 = lim_mix(T, 1), lim_mix(T, 2)
    p1[0, CEIL], p1[1, CEIL] = p0[0, CEIL] / 40.0, p0[1, CEIL] * 40.0    # steep ramps, down and up
    twin = Twin(T, B, W)
    twin.set_params(p0, ramp=False)
    x = hot_noise(T, 3 * B, 12, np.maximum(p0[:, CEIL], p1[:, CEIL]))
    ys, ceils = [], []
    for k in range(3):
        if k == 1:
            twin.set_params(p1)
        ceils.append(np.array(sample_params(twin.cur, twin.tgt, mix_ramp(B) if twin.pending else None, B)[CEIL]))  # (a copy)
        ys.append(twin.process(x[:, k * B:(k + 1) * B])[0])
    y, ceil = np.concatenate(ys, axis=1), np.concatenate(ceils, axis=1)
    assert not (y[:, :D] != 0).any()
    assert (np.abs(y[:, D:]) <= ceil[:, :-D]).all()                    # the ceiling in force when the sample came in
    assert np.array_equal(twin.cur, p1) and not twin.pending
    mid = ceil[0, B + B // 2]
    assert p1[0, CEIL] < mid < p0[0, CEIL]


# ---- the rule ----------------------------------------------------------------------------------------------------
def test_every_spoilt_field_is_refused_and_the_first_is_named():
    up = lambda v: np.nextafter(f32(v), f32(np.inf))                   # noqa: E731
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))                # noqa: E731
    good = lim_mix(8, 1)
    assert first_refused(good) is None
    cases = [(np.nan, DRIVE), (np.inf, DRIVE), (f32(-1e-30), DRIVE), (up(2.0 ** 32), DRIVE),
             (np.nan, CEIL), (0.0, CEIL), (down(2.0 ** -32), CEIL), (up(2.0 ** 32), CEIL), (-1.0, CEIL), (np.inf, CEIL),
             (np.nan, REL), (f32(-1e-30), REL), (up(1.0), REL), (np.inf, REL)]
    for n, (value, field) in enumerate(cases):
        bad = good.copy()
        track = n % 7
        bad[track, field] = value
        bad[track + 1, DRIVE] = np.nan                                # a later offender is not the one named
        assert first_refused(bad) == track * FIELDS + field, (value, field)
    edges = np.array([[0.0, 2.0 ** -32, 0.0], [2.0 ** 32, 2.0 ** 32, 1.0], [-0.0, 1.0, -0.0]], np.float32)
    assert first_refused(edges) is None


def test_limiter_params():
    r = limiter_params(-1.0, 100.0, 6.0)
    assert r.shape == (3,) and r.dtype == np.float32
    want = np.array([10.0 ** 0.3, 10.0 ** -0.05, 1.0 - np.exp(-1.0 / 4800.0)], np.float64).astype(np.float32)
    assert np.array_equal(r, want)
    assert [v.hex() for v in r.astype(np.float64)] == ["0x1.fec9820000000p+0", "0x1.c8520a0000000p-1", "0x1.b4dc740000000p-13"]
    assert np.array_equal(limiter_params(0.0, 0.0), np.array([1, 1, 1], np.float32))
    t = limiter_params([-1.0, -3.0], 50.0, [0.0, 12.0])
    assert t.shape == (2, 3) and t[0, DRIVE] == 1.0 and t[0, REL] == t[1, REL] and first_refused(t) is None
    with pytest.raises(ValueError):
        limiter_params(-1.0, -5.0)


# ---- the library without a GPU -----------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 6, 1), (-1, 512, 6, 1), (4, 0, 6, 1), (4, 512, 1, 1), (4, 512, 9, 1), (4, 512, -3, 1),
                 (4, 512, 6, 0), (4, 512, 6, 3), (6, 512, 6, 4), (128, 512, 6, 128), (3, 512, 6, 2)):
        assert lib.gab_lim_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_lim_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_lim_create(None, 4, 512, 6, 1) == bad
    assert b"gab_lim_create" in lib.gab_last_error() and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_lim_process(None, None, None, None, None), b"gab_lim_process"),
                       (lambda: lib.gab_lim_process_batch(None, None, None, None, 1, None), b"gab_lim_process_batch"),
                       (lambda: lib.gab_lim_set_params(None, None, 1, None), b"gab_lim_set_params"),
                       (lambda: lib.gab_lim_set_params_tracks(None, None, 0, 1, 1, None), b"gab_lim_set_params_tracks"),
                       (lambda: lib.gab_lim_params(None, None, None, None), b"gab_lim_params"),
                       (lambda: lib.gab_lim_state(None, None, None, None, None), b"gab_lim_state"),
                       (lambda: lib.gab_lim_latency(None, None), b"gab_lim_latency"),
                       (lambda: lib.gab_lim_reset(None, None), b"gab_lim_reset"),
                       (lambda: lib.gab_lim_destroy(None), b"gab_lim_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_limiter_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_lim_create(C.byref(h), 4, 512, 6, 2)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_lim_create" in text


def test_limiter_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "LimiterPlan" in g.__all__ and callable(g.LimiterPlan) and "limiter_params" in g.__all__
    assert issubclass(g.LimiterPlan, g.ops._TrackPlan)
    for name in ("set_params", "reset", "process", "process_batch", "params", "state", "prepare", "launch", "close"):
        assert hasattr(g.LimiterPlan, name), name
    assert g.LimiterPlan.FIELDS == ("drive", "ceil", "rel")
