"""The mix-bus plan (gab_mix_*) without a GPU: the references the GPU tests compare against, shown to be what they
claim to be; known answers; the stereo convenience; argument checks and exports.

    fma32              round32(a*b + c) with ONE rounding, vectorised: the float64 product is exact (24 + 24 bits), the
                       float64 sum is not, so its exact residual (TwoSum) decides the cases where the float64 sum sits
                       exactly half way between two float32 values.  Held against exact rational arithmetic.
    mix_ramp           r[s] = (s + 1) / B in float64, rounded once: the plan's table.
    mix_reference_f32  the contract of include/gab_c_api.h, parametrised by (leaf_tracks, group_leaves): chains of fma32
                       over a leaf's tracks, the leaves of a group added in ascending order in float32, then the groups.
                       What mix_kernel + mix_groups_kernel must equal bit for bit.
    mix_reference_f64  sum_t g64 x64, with g64 the ramp in float64 on the float32 inputs: the truth.

The a-priori bound of the tree, per output: |err| <= (leaf_tracks + n_leaves + 3) * 2^-24 * sum_t |g x| (the chain's
roundings, at most n_leaves adds, the ramp's two roundings and one to spare).  Derived, not measured; the figures of every
case: pytest -s.

The tests of the references themselves (fma32, the bound, the known answers) need nothing of the library and pass on
any commit; what fails without the feature is the stereo law, the argument checks, the runtime-mode refusal, the export
test here, and every test of tests/test_mix_gpu.py.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from plan_helpers import bits

EPS = 2.0 ** -24


def fma32(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)      # exact
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                        # p + c = s + e exactly
        r = s.astype(np.float32)                             # nearest-even on s
        diff = s - r.astype(np.float64)                      # exact
        other = np.nextafter(r, np.where(diff > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        half = (diff != 0) & (s == (r.astype(np.float64) + other.astype(np.float64)) * 0.5)
        beyond = half & (e != 0) & ((e > 0) == (diff > 0))   # the true sum is past the half-way point
    # An operand that is not finite makes s an infinity or a NaN, which is fmaf's own answer; the residual means nothing
    # there (inf - inf), and without this line fma32(+inf, 1, 0) came out as FLT_MAX (tests/test_edges_host.py).
    return np.where(np.isfinite(s) & beyond, other, r).astype(np.float32)


def fma32_double_rounded(a, b, c):
    """What fma32 must NOT be: the float64 sum rounded to 53 bits, then to 24."""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def round32_exact(q):
    """A Fraction to the nearest float32, ties to even (normal and subnormal range)."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    n = q / quantum
    f = n.numerator // n.denominator
    rem = n - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return np.float32(sign * float(f * quantum))


def mix_ramp(B):
    return ((np.arange(B, dtype=np.float64) + 1.0) / float(B)).astype(np.float32)


def mix_reference_f32(x, current, target, r, leaf_tracks, group_leaves):
    """x [T][B], current / target [T][M] float32; r: the ramp table [B] on a buffer with a pending ramp, else None.
    Returns [M][B] float32.  All leaves run side by side; within one the tracks ascend."""
    x = np.asarray(x, np.float32)
    cur, tgt = np.asarray(current, np.float32), np.asarray(target, np.float32)
    T, B = x.shape
    M = tgt.shape[1]
    L, G = int(leaf_tracks), int(group_leaves)
    n_leaves = (T + L - 1) // L
    starts = np.arange(n_leaves) * L
    acc = np.zeros((n_leaves, M, B), np.float32)
    d = tgt - cur                                            # float32: one rounding
    for j in range(L):
        k = int(np.count_nonzero(starts + j < T))            # only the last leaf can be short
        if k == 0:
            break
        t = starts[:k] + j
        if r is None:
            g = tgt[t][:, :, None]
        else:
            g = fma32(d[t][:, :, None], np.asarray(r, np.float32)[None, None, :], cur[t][:, :, None])
        acc[:k] = fma32(g, x[t][:, None, :], acc[:k])
    n_groups = (n_leaves + G - 1) // G
    out = None
    for gi in range(n_groups):
        grp = acc[gi * G].copy()
        for leaf in range(gi * G + 1, min((gi + 1) * G, n_leaves)):
            grp = grp + acc[leaf]                            # float32 add
        out = grp if out is None else out + grp
    assert out.dtype == np.float32
    return out


class Twin:
    """The plan's state machine on the host: current, target, a pending ramp; process() is mix_reference_f32 with the
    form (leaf_tracks, group_leaves) it is given, which a device test holds against plan.form."""

    def __init__(self, tracks, bufsize, buses, leaf_tracks, group_leaves):
        self.T, self.B, self.M = tracks, bufsize, buses
        self.L, self.G = leaf_tracks, group_leaves
        self.cur = np.zeros((self.T, self.M), np.float32)
        self.tgt = np.zeros((self.T, self.M), np.float32)
        self.pending = False

    def set_gains(self, g, ramp=True, first=0):
        n = g.shape[0]
        self.tgt[first:first + n] = g
        if ramp:
            self.pending = True
        else:
            self.cur[first:first + n] = g

    def reset(self):
        self.cur[:] = self.tgt
        self.pending = False

    def process(self, x):
        y = mix_reference_f32(x, self.cur, self.tgt, mix_ramp(self.B) if self.pending else None, self.L, self.G)
        if self.pending:
            self.cur[:] = self.tgt
            self.pending = False
        return y


def mix_gains_f64(current, target, r):
    cur, tgt = np.asarray(current, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    if r is None:
        return tgt[:, :, None]
    return cur[:, :, None] + (tgt - cur)[:, :, None] * np.asarray(r, np.float32).astype(np.float64)[None, None, :]


def mix_reference_f64(x, current, target, r):
    """(sum_t g x, sum_t |g x|), each [M][B] float64."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    g = mix_gains_f64(current, target, r)
    if r is None:
        g2 = g[:, :, 0]
        return g2.T @ x64, np.abs(g2).T @ np.abs(x64)
    return np.einsum("tms,ts->ms", g, x64), np.einsum("tms,ts->ms", np.abs(g), np.abs(x64))


def tree_bound(T, leaf_tracks):
    return (leaf_tracks + (T + leaf_tracks - 1) // leaf_tracks + 3) * EPS


def noise(T, B, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, B)).astype(np.float32)


def gains(T, M, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (T, M)).astype(np.float32)


# ---- fma32 ----------------------------------------------------------------------------------------------------
HALF_WAY = [
    # a*b = 2^-24 + 2^-60: the float64 sum 1 + 2^-24 is a tie that goes to 1.0; the truth is past it, 1 + 2^-23
    (4097 * 2.0 ** -30, 16773121 * 2.0 ** -30, 1.0),
    (-4097 * 2.0 ** -30, 16773121 * 2.0 ** -30, -1.0),
    # the same just below the tie of an odd neighbour: 1 + 2^-23 + 2^-24 - 2^-60 must go down to 1 + 2^-23
    (-4097 * 2.0 ** -30, 16773121 * 2.0 ** -30, 1.0 + 2.0 ** -23 + 2.0 ** -23),
    # exact ties (residual zero) stay nearest-even: 1 + 2^-24 -> 1, 1 + 3 * 2^-24 -> 1 + 2^-22
    (2.0 ** -12, 2.0 ** -12, 1.0),
    (3 * 2.0 ** -12, 2.0 ** -12, 1.0),
]


def test_half_way_case_is_what_the_issue_says():
    a, b, c = HALF_WAY[0]
    assert np.float32(a) == a and np.float32(b) == b
    assert Fraction(a) * Fraction(b) == Fraction(2) ** -24 + Fraction(2) ** -60
    assert round32_exact(Fraction(a) * Fraction(b) + Fraction(c)) == np.float32(1.0 + 2.0 ** -23)
    assert fma32_double_rounded(a, b, c) == np.float32(1.0)
    assert fma32(a, b, c) == np.float32(1.0 + 2.0 ** -23)


def test_fma32_is_one_rounding():
    rng = np.random.RandomState(1)
    n = 4000
    a = rng.uniform(-2, 2, n).astype(np.float32)
    b = rng.uniform(-2, 2, n).astype(np.float32)
    c = (rng.uniform(-2, 2, n) * 2.0 ** rng.randint(-30, 4, n)).astype(np.float32)
    # products that nearly cancel c, and products far below c's last bit
    c[:1000] = (-(a[:1000].astype(np.float64) * b[:1000])).astype(np.float32)
    a[1000:1500] *= np.float32(2.0 ** -25)
    for k, (x, y, z) in enumerate(HALF_WAY):
        a[2000 + k], b[2000 + k], c[2000 + k] = x, y, z
    got = fma32(a, b, c)
    want = np.array([round32_exact(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:10]
    # the cases bite: the double-rounded form fails at least one of them
    dr = fma32_double_rounded(a, b, c)
    assert (bits(dr) != bits(want)).any()


# ---- the reference against float64 ------------------------------------------------------------------------------
BOUND_CASES = [(8192, 512, 16, 64, 1), (8192, 512, 16, 512, 1), (8192, 512, 16, 32, 8), (1024, 512, 2, 32, 8),
               (1000, 100, 5, 32, 8), (1000, 100, 5, 64, 1), (300, 64, 64, 64, 4)]


@pytest.mark.parametrize("T,B,M,L,G", BOUND_CASES)
@pytest.mark.parametrize("ramp", [False, True])
def test_reference_is_within_the_tree_bound_of_float64(T, B, M, L, G, ramp):
    x, cur, tgt = noise(T, B, T + B), gains(T, M, T + M), gains(T, M, T + M + 1)
    r = mix_ramp(B) if ramp else None
    y = mix_reference_f32(x, cur, tgt, r, L, G)
    y64, mag = mix_reference_f64(x, cur, tgt, r)
    err = np.abs(y.astype(np.float64) - y64)
    bound = tree_bound(T, L) * mag
    peak = np.abs(y64).max()
    print("mix reference %d x %d x %d, leaves of %d, groups of %d, %s: worst err / bound %.3g, err / peak %.3g"
          % (T, B, M, L, G, "ramp" if ramp else "steady", (err / bound).max(), err.max() / peak))
    assert (err <= bound).all()
    assert err.max() <= 1e-5 * peak


# ---- the reference against itself -----------------------------------------------------------------------------
def mix_reference_loops(x, cur, tgt, r, L, G):
    """The contract as written, one output at a time (small shapes only)."""
    T, B = x.shape
    M = tgt.shape[1]
    out = np.zeros((M, B), np.float32)
    for m in range(M):
        for s in range(B):
            groups = []
            for g0 in range(0, T, L * G):
                leaves = []
                for l0 in range(g0, min(g0 + L * G, T), L):
                    acc = np.float32(0.0)
                    for t in range(l0, min(l0 + L, T)):
                        g = tgt[t, m] if r is None else fma32(np.float32(tgt[t, m] - cur[t, m]), r[s], cur[t, m])
                        acc = fma32(g, x[t, s], acc)
                    leaves.append(np.float32(acc))
                v = leaves[0]
                for q in leaves[1:]:
                    v = np.float32(v + q)
                groups.append(v)
            v = groups[0]
            for q in groups[1:]:
                v = np.float32(v + q)
            out[m, s] = v
    return out


@pytest.mark.parametrize("T,L,G", [(70, 32, 2), (64, 32, 2), (97, 32, 2), (5, 32, 8), (33, 8, 3), (50, 8, 1), (1, 4, 4)])
def test_short_leaves_and_groups(T, L, G):
    """A short last leaf, a short last group, fewer tracks than a leaf: the vectorised reference is the contract as
    written."""
    B, M = 3, 2
    x, cur, tgt = noise(T, B, T), gains(T, M, T + 1), gains(T, M, T + 2)
    for r in (None, mix_ramp(B)):
        assert np.array_equal(bits(mix_reference_f32(x, cur, tgt, r, L, G)), bits(mix_reference_loops(x, cur, tgt, r, L, G)))


def test_steady_form_is_the_ramp_form_at_rest():
    T, B, M = 200, 64, 3
    x, g = noise(T, B, 1), gains(T, M, 2)
    g[np.abs(g) < 1e-3] = 0.5                      # away from zero
    assert np.array_equal(bits(mix_reference_f32(x, g, g, None, 32, 8)), bits(mix_reference_f32(x, g, g, mix_ramp(B), 32, 8)))


def test_a_ramp_ends_at_r_equal_one():
    """r[B-1] is exactly 1, so the last sample of a ramp buffer is mixed with fl(fl(target - current) + current): the
    target to an ulp, which is why the plan then sets current := target itself."""
    for B in (1, 3, 64, 100, 512, 513, 2048):
        r = mix_ramp(B)
        assert r[-1] == np.float32(1.0) and (np.diff(r) > 0).all() and r[0] == np.float32(1.0 / B)
    T, B, M = 100, 16, 2
    x, cur, tgt = noise(T, B, 3), gains(T, M, 4), gains(T, M, 5)
    y = mix_reference_f32(x, cur, tgt, mix_ramp(B), 32, 8)
    last = ((tgt - cur) + cur).astype(np.float32)
    assert np.array_equal(bits(y[:, -1]), bits(mix_reference_f32(x, last, last, None, 32, 8)[:, -1]))


# ---- known answers ----------------------------------------------------------------------------------------------
def one_hot_case(T, B, M, seed):
    """(x, gains, route): bus m carries track route[m], every other gain is zero."""
    rng = np.random.RandomState(seed)
    route = rng.choice(T, M, replace=False)
    g = np.zeros((T, M), np.float32)
    g[route, np.arange(M)] = 1.0
    return noise(T, B, seed + 1), g, route


def small_integer_case(T, B, M, seed):
    """Gains in -3..3, samples in -15..15: every partial sum is an integer below 2^24 for T <= 2^18."""
    rng = np.random.RandomState(seed)
    g = rng.randint(-3, 4, (T, M)).astype(np.float32)
    x = rng.randint(-15, 16, (T, B)).astype(np.float32)
    want = (g.astype(np.int64).T @ x.astype(np.int64))
    assert np.abs(g.astype(np.int64)).T.dot(np.abs(x.astype(np.int64))).max() < 2 ** 24
    return x, g, want.astype(np.float32)


@pytest.mark.parametrize("L,G", [(32, 8), (64, 4), (7, 3)])
def test_known_answers(L, G):
    x, g, route = one_hot_case(300, 50, 6, 11)
    assert np.array_equal(bits(mix_reference_f32(x, g, g, None, L, G)), bits(x[route]))
    x, g, want = small_integer_case(1000, 40, 5, 12)
    assert np.array_equal(mix_reference_f32(x, g, g, None, L, G), want)


# ---- set_stereo -----------------------------------------------------------------------------------------------
def test_stereo_law():
    from gpuaudiobench_amd import MixPlan
    rng = np.random.RandomState(5)
    db, pan = rng.uniform(-60, 12, 1000), rng.uniform(-1, 1, 1000)
    g = MixPlan.stereo_gains(db, pan)
    assert g.shape == (1000, 2) and g.dtype == np.float32
    lin = 10.0 ** (db / 20.0)
    power = g[:, 0].astype(np.float64) ** 2 + g[:, 1].astype(np.float64) ** 2
    assert np.abs(power / lin ** 2 - 1.0).max() <= 4 * EPS          # two roundings, squared
    c = MixPlan.stereo_gains(0.0, 0.0)
    assert c.shape == (2,) and abs(20 * np.log10(c[0]) + 3.0103) < 1e-3 and c[0] == c[1]
    left, right = MixPlan.stereo_gains(0.0, -1.0), MixPlan.stereo_gains(0.0, 1.0)
    assert left[0] == 1.0 and left[1] == 0.0
    assert right[1] == 1.0 and abs(right[0]) <= np.cos(np.pi / 2) * 1.0000001      # cos(pi/2) in float64: 6e-17
    with pytest.raises(ValueError):
        MixPlan.stereo_gains(0.0, 1.5)


# ---- the library without a GPU --------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 2), (-1, 512, 2), (4, 0, 2), (4, -5, 2), (4, 512, 0), (4, 512, 65), (4, 512, -1)):
        assert lib.gab_mix_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_mix_create" in lib.gab_last_error()
        assert not h.value
    assert lib.gab_mix_create(None, 4, 512, 2) == bad
    assert b"gab_mix_create" in lib.gab_last_error() and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_mix_process(None, None, None, 0, None), b"gab_mix_process"),
                       (lambda: lib.gab_mix_process_batch(None, None, None, 1, 0, None), b"gab_mix_process_batch"),
                       (lambda: lib.gab_mix_set_gains(None, None, 1, None), b"gab_mix_set_gains"),
                       (lambda: lib.gab_mix_set_gains_tracks(None, None, 0, 1, 1, None), b"gab_mix_set_gains_tracks"),
                       (lambda: lib.gab_mix_gains(None, None, None, None), b"gab_mix_gains"),
                       (lambda: lib.gab_mix_form(None, None, None), b"gab_mix_form")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()
    assert lib.gab_mix_reset(None, None) == bad
    assert b"gab_mix_reset" in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()
    assert lib.gab_mix_destroy(None) == bad
    assert b"gab_mix_destroy" in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_mix_plan_refuses_the_runtime_mode_the_other_plans_refuse():
    import os
    import subprocess
    import sys
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_mix_create(C.byref(h), 4, 512, 2)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AMD_DIRECT_DISPATCH="0"), capture_output=True,
                       text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "gab_mix_create" in text


def test_mix_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "MixPlan" in g.__all__ and callable(g.MixPlan)
    for name in ("set_gains", "set_stereo", "stereo_gains", "reset", "process", "process_batch", "gains", "form",
                 "prepare", "launch", "close"):
        assert hasattr(g.MixPlan, name), name
    assert g._capi.MIX_TRACK_MAJOR == 0 and g._capi.MIX_SAMPLE_MAJOR == 1
