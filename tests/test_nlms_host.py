"""The nlms plan's contract (include/gab_c_api.h, gab_nlms_*) without a GPU: tests/nlms_twin.py, the restatement the
device is held to bit for bit in tests/test_nlms_gpu.py, against known answers: a delay through one-hot taps, the tree
as written, any cut of a stream, the identification of a known response, float64, containment of what is not finite,
a tail through the subnormals, the ramp, the rule."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from nlms_twin import (EPS_MAX, EPS_MIN, F32, NlmsTwin, chain32, dot32, first_bad_tap, first_refused, nlms_params,
                       not_finite, tree32)
from plan_helpers import bits
from test_mix_host import fma32, mix_ramp, round32_exact

U = 2.0 ** -24


def noise(T, n, seed, scale=0.25):
    return (scale * np.random.default_rng(seed).standard_normal((T, n))).astype(F32)


def resume(twin, B):
    """A twin of another buffer size that goes on where `twin` stands."""
    t = NlmsTwin(twin.T, B, twin.L, twin.wide)
    t.cur, t.tgt, t.pending = twin.cur.copy(), twin.tgt.copy(), twin.pending
    t.w, t.hist = twin.w.copy(), twin.hist.copy()
    return t


def adapting(T, B, L, mu=0.5, eps=1e-6, wide=False):
    t = NlmsTwin(T, B, L, wide)
    t.set_params(np.tile(np.array([mu, eps], F32), (T, 1)), ramp=False)
    return t


# ---- the filter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 128, 512])
def test_one_hot_taps_delay_the_reference_bit_for_bit(L):
    ks = [k for k in (0, 63, 64, L - 1) if k < L]
    T, n = len(ks), L + 70
    x, d = noise(T, n, 1), noise(T, n, 2)
    w = np.zeros((T, L), F32)
    for t, k in enumerate(ks):
        w[t, k] = 1.0
    twin = NlmsTwin(T, n, L)                                          # mu = 0: no adaptation
    twin.set_taps(w)
    err, est = twin.process(d, x)
    for t, k in enumerate(ks):
        want = np.concatenate([np.zeros(k, F32), x[t, :n - k]])
        assert np.array_equal(bits(est[t]), bits(want)), k
        assert np.array_equal(bits(err[t]), bits((d[t] - want).astype(F32))), k
    assert np.array_equal(bits(twin.w), bits(w))
    assert np.array_equal(bits(twin.hist), bits(x[:, n - (L - 1):]))  # the last L - 1 samples, oldest first


def tree_as_written(v):
    """32 sums of (2i, 2i + 1), then 16, down to 1: scalars, one rounded addition each."""
    v = [F32(a) for a in v]
    while len(v) > 1:
        v = [F32(v[2 * i] + v[2 * i + 1]) for i in range(len(v) // 2)]
    return v[0]


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_the_tree_is_the_tree_as_written_and_within_its_bound_of_the_exact_sum(R):
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((5, 64 * R)) * np.exp(rng.uniform(-20, 20, (5, 64 * R)))).astype(F32)
    X = rng.standard_normal((5, 64 * R)).astype(F32)
    got = dot32(w, X)
    for t in range(5):
        acc = [F32(w[t, l] * X[t, l]) for l in range(64)]
        for q in range(1, R):
            acc = [fma32(w[t, 64 * q + l], X[t, 64 * q + l], acc[l]) for l in range(64)]
        assert bits(got[t]) == bits(tree_as_written(acc)), t
        assert np.array_equal(bits(chain32(w[t].reshape(R, 64), X[t].reshape(R, 64))), bits(np.array(acc, F32)))
        # R roundings in the chain and 6 in the tree touch every term at most once each
        terms = [float(a) * float(b) for a, b in zip(w[t], X[t])]
        bound = ((1 + U) ** (R + 6) - 1) * math.fsum(abs(v) for v in terms)
        assert abs(float(got[t]) - math.fsum(terms)) <= bound, t
    assert bits(tree32(np.arange(64, dtype=F32))) == bits(F32(2016))


# ---- any cut is the whole stream -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole(L, n):
    T = 2
    x, d = noise(T, n, 11), noise(T, n, 12)
    twin = adapting(T, n, L)
    err, est = twin.process(d, x)
    return x, d, err, est, twin


@pytest.mark.parametrize("B", [1, 63, 64, 65, 100, 512])
def test_any_cut_into_buffers_and_batches_is_the_whole_stream(B):
    L = 128                                                           # 63, 64, 65 and 100 are shorter than L - 1
    nb = max(2, 300 // B)
    n = nb * B
    x, d, err, est, ref = whole(L, n)
    T = x.shape[0]
    cut = lambda a: a.reshape(T, nb, B).transpose(1, 0, 2)            # noqa: E731
    per, bat = adapting(T, B, L), adapting(T, B, L)
    outs = [per.process(dk, xk) for dk, xk in zip(cut(d), cut(x))]
    half = nb // 2
    e1, y1 = bat.process_batch(cut(d)[:half], cut(x)[:half])
    e2, y2 = bat.process_batch(cut(d)[half:], cut(x)[half:])
    for e, y in ((np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])),
                 (np.concatenate([e1, e2]), np.concatenate([y1, y2]))):
        assert np.array_equal(bits(e), bits(cut(err))) and np.array_equal(bits(y), bits(cut(est)))
    for t in (per, bat):
        assert np.array_equal(bits(t.w), bits(ref.w)) and np.array_equal(bits(t.hist), bits(ref.hist))
    assert np.abs(ref.w).max() > 0.01                                 # and the taps moved


def test_a_new_plan_returns_the_input_and_plus_zero():
    T, B = 3, 70
    d, x = noise(T, B, 4, 1e3), noise(T, B, 5, 1e3)
    d[0, 3], d[1, 7], d[2, 0] = -0.0, np.inf, np.nan
    twin = NlmsTwin(T, B, 64)
    err, est = twin.process(d, x)
    assert np.array_equal(bits(err), bits(d)) and not bits(est).any()
    assert not bits(twin.w).any() and np.array_equal(bits(twin.hist), bits(x[:, B - 63:]))


# ---- identification ------------------------------------------------------------------------------------------------
CASES = {64: (4096, 0.5), 128: (4096, 0.5), 256: (8192, 1.0), 512: (8192, 1.0)}


def response(L):
    """A decaying resonance, the same for every L."""
    k = np.arange(L, dtype=np.float64)
    return np.exp(-k / 8.0) * np.cos(0.9 * k)


@functools.lru_cache(maxsize=None)
def identified(L, wide):
    n, mu = CASES[L]
    x = (0.25 * np.random.default_rng(7).standard_normal(n)).astype(F32)[None]
    h = response(L)
    d = np.convolve(x[0].astype(np.float64), h)[:n].astype(F32)[None]          # noise-free
    twin = adapting(1, n, L, mu=mu, eps=1e-6, wide=wide)
    err, _ = twin.process(d, x)
    return d, err, twin.w[0].astype(np.float64), h


@pytest.mark.parametrize("L", [64, 128, 256, 512])
def test_a_known_response_is_identified_to_minus_80_db(L):
    """The condition: misalignment |w - h|^2 / |h|^2 <= -80 dB after 4 096 samples at mu = 0.5 (L = 64, 128), after
    8 192 at mu = 1 (L = 256, 512).  The float32 restatement reaches -138.2, -125.2, -130.6 and -117.1 dB."""
    _, _, w, h = identified(L, False)
    mis = 10.0 * np.log10(((w - h) ** 2).sum() / (h ** 2).sum())
    print("L = %d: misalignment %.1f dB" % (L, mis))
    assert mis <= -80.0, mis


@pytest.mark.parametrize("L", [64, 128, 256, 512])
def test_float32_is_within_the_projects_bound_of_float64(L):
    """max |e32 - e64| <= 1e-5 of d's peak, the project's bound for its float32 paths; reached: 3.3e-7, 4.7e-7, 4.5e-7, 5.3e-7."""
    d, e32, _, _ = identified(L, False)
    _, e64, _, _ = identified(L, True)
    worst = np.abs(e32.astype(np.float64) - e64).max() / np.abs(d).max()
    print("L = %d: max |e32 - e64| = %.2e of d's peak" % (L, worst))
    assert worst <= 1e-5, worst


# ---- what is not finite stays where it entered ----------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 256])
def test_a_nan_in_the_reference_is_in_the_outputs_for_L_samples_and_never_in_a_tap(L):
    T, at, n = 2, 100, 100 + L + 150
    x, d = noise(T, n, 21), noise(T, n, 22)
    dirty = x.copy()
    dirty[0, at] = np.nan
    twin = adapting(T, n, L)
    err, est = twin.process(d, dirty)
    bad = np.zeros((T, n), bool)
    bad[0, at:at + L] = True
    assert np.array_equal(not_finite(err), bad) and np.array_equal(not_finite(est), bad)
    assert twin.skipped == L and not not_finite(twin.w).any()
    # a twin that simply skipped those updates: the clean stream with mu = 0 on those L samples
    a = adapting(T, at, L)
    ea, _ = a.process(d[:, :at], x[:, :at])
    b = resume(a, L)
    held = b.tgt.copy()
    held[0, 0] = 0.0
    b.set_params(held, ramp=False)
    b.process(d[:, at:at + L], x[:, at:at + L])
    c = resume(b, n - at - L)
    c.set_params(a.tgt, ramp=False)
    ec, _ = c.process(d[:, at + L:], x[:, at + L:])
    assert np.array_equal(twin.w, c.w)                                # by value: a zero's sign may differ under mu = 0
    assert np.array_equal(bits(err[:, :at]), bits(ea)) and np.array_equal(bits(err[:, at + L:]), bits(ec))
    clean = adapting(1, n, L)                                         # the neighbour: as if it ran alone
    e1, y1 = clean.process(d[1:], x[1:])
    assert np.array_equal(bits(err[1:]), bits(e1)) and np.array_equal(bits(est[1:]), bits(y1))
    assert np.array_equal(bits(twin.w[1:]), bits(clean.w))


def test_an_infinity_in_the_input_is_in_one_sample_of_the_error_and_never_in_a_tap():
    T, L, at, n = 2, 64, 40, 200
    x, d = noise(T, n, 23), noise(T, n, 24)
    dirty = d.copy()
    dirty[1, at] = np.inf
    twin = adapting(T, n, L)
    err, est = twin.process(dirty, x)
    bad = np.zeros((T, n), bool)
    bad[1, at] = True
    assert np.array_equal(not_finite(err), bad) and not not_finite(est).any()
    assert twin.skipped == 1 and not not_finite(twin.w).any()
    a = adapting(T, at, L)
    a.process(d[:, :at], x[:, :at])
    b = resume(a, 1)
    held = b.tgt.copy()
    held[1, 0] = 0.0
    b.set_params(held, ramp=False)
    b.process(d[:, at:at + 1], x[:, at:at + 1])
    c = resume(b, n - at - 1)
    c.set_params(a.tgt, ramp=False)
    ec, yc = c.process(d[:, at + 1:], x[:, at + 1:])
    assert np.array_equal(twin.w, c.w)
    assert np.array_equal(bits(err[:, at + 1:]), bits(ec)) and np.array_equal(bits(est[:, at + 1:]), bits(yc))


def subnormal_tail(T=2, L=64, n=704):
    """x and d fading by 2^(-n/4) through the subnormals to zero; eps = 2^-100."""
    fade = np.exp2(-np.arange(n) / 4.0)
    x = (noise(T, n, 31).astype(np.float64) * fade).astype(F32)
    d = (noise(T, n, 32).astype(np.float64) * fade).astype(F32)
    return x, d, np.tile(np.array([0.5, 2.0 ** -100], F32), (T, 1))


def test_a_tail_through_the_subnormals_stays_finite():
    x, d, p = subnormal_tail()
    T, n = x.shape
    assert not x[:, -64:].any() and not d[:, -64:].any()             # the tail ends in zeros
    twin = NlmsTwin(T, n, 64)
    twin.set_params(p, ramp=False)
    err, est = twin.process(d, x)
    assert not not_finite(err).any() and not not_finite(est).any() and not not_finite(twin.w).any()
    assert twin.skipped == 0
    tiny = lambda a: int(((a != 0) & (np.abs(a) < 2.0 ** -126)).sum())             # noqa: E731
    counts = (tiny(x), tiny(d), tiny(err), tiny(est))
    print("subnormals in x, d, err, est:", counts)
    assert counts == SUBNORMALS


SUBNORMALS = (190, 188, 182, 183)          # the restatement's own count, pinned


# ---- the ramp -------------------------------------------------------------------------------------------------------
def test_a_ramped_set_is_the_per_sample_formula():
    T, B, L = 2, 50, 64
    x, d = noise(T, 2 * B, 41), noise(T, 2 * B, 42)
    p0 = np.array([[0.25, 1e-3], [1.0, 1e-6]], F32)
    p1 = np.array([[1.5, 1e-5], [0.0, 0.5]], F32)
    twin = NlmsTwin(T, B, L)
    twin.set_params(p0, ramp=False)
    twin.set_params(p1)
    assert np.array_equal(bits(twin.cur), bits(p0)) and np.array_equal(bits(twin.tgt), bits(p1))
    outs = [twin.process(d[:, :B], x[:, :B]), twin.process(d[:, B:], x[:, B:])]
    assert np.array_equal(bits(twin.cur), bits(p1)) and not twin.pending
    # one sample a call, every row worked out exactly and set at once
    r = mix_ramp(B)
    single = NlmsTwin(T, 1, L)
    for s in range(2 * B):
        row = p1
        if s < B:
            diff = (p1 - p0).astype(F32)
            row = np.array([[round32_exact(Fraction(float(diff[t, f])) * Fraction(float(r[s])) + Fraction(float(p0[t, f])))
                             for f in (0, 1)] for t in range(T)], F32)
        single.set_params(row, ramp=False)
        e, y = single.process(d[:, s:s + 1], x[:, s:s + 1])
        k, i = divmod(s, B)
        assert np.array_equal(bits(e[:, 0]), bits(outs[k][0][:, i])), s
        assert np.array_equal(bits(y[:, 0]), bits(outs[k][1][:, i])), s
    assert np.array_equal(bits(single.w), bits(twin.w))
    assert bits(r[B - 1]) == bits(F32(1.0))                           # the ramp ends on the target's step


# ---- the rule -------------------------------------------------------------------------------------------------------
def test_the_rule_on_every_spoilt_field():
    up = lambda v, to=np.inf: np.nextafter(F32(v), F32(to))            # noqa: E731
    good = np.tile(nlms_params(0.5, -60.0, 64), (6, 1))
    assert first_refused(good) is None
    edges = np.array([[-0.0, EPS_MIN], [2.0, EPS_MAX], [0.0, 1.0], [2.0 ** -149, 2.0 ** -126]], F32)
    assert first_refused(edges) is None                               # -0.0 is taken, and every edge itself
    cases = [((2, 0), up(2.0, 3.0)), ((3, 0), np.nan), ((1, 0), np.inf), ((4, 0), -np.inf), ((0, 0), -2.0 ** -149),
             ((2, 1), 0.0), ((3, 1), 2.0 ** -127), ((5, 1), up(2.0 ** 64)), ((0, 1), np.nan), ((1, 1), np.inf),
             ((4, 1), -1.0)]
    for (t, f), v in cases:
        bad = good.copy()
        bad[t, f] = v
        if t + 1 < len(bad):
            bad[t + 1, 1] = np.nan                                    # the FIRST offender is named
        assert first_refused(bad) == 2 * t + f, (t, f, v)
        twin = NlmsTwin(len(bad), 8, 64)
        with pytest.raises(ValueError, match="track %d field %d" % (t, f)):
            twin.set_params(bad)
        assert np.array_equal(bits(twin.tgt), bits(twin.cur)) and not twin.pending
    w = np.zeros((3, 64), F32)
    assert first_bad_tap(w) is None
    w[1, 5], w[2, 0] = np.nan, np.inf
    assert first_bad_tap(w) == 64 + 5
    twin = NlmsTwin(3, 8, 64)
    with pytest.raises(ValueError, match="track 1 tap 5"):
        twin.set_taps(w)
    assert not twin.w.any()


def test_nlms_params_rows():
    from gpuaudiobench_amd import nlms_params as made
    row = made()                                                      # step 0.5, a floor of -60 dB, 64 taps
    assert row.dtype == np.float32 and row.shape == (2,)
    assert bits(row[0]) == bits(F32(0.5)) and bits(row[1]) == bits(round32_exact(Fraction(64, 10 ** 6)))
    assert bits(row[1]) == 0x388637BD
    table = made(step=[0.25, 1.0], floor_db=-50.0, taps=[128, 512])
    assert table.shape == (2, 2) and table.dtype == np.float32
    assert bits(table[0, 1]) == bits(round32_exact(Fraction(128, 10 ** 5)))
    assert bits(table[1, 1]) == bits(round32_exact(Fraction(512, 10 ** 5)))
    assert np.array_equal(bits(table[:, 0]), bits(np.array([0.25, 1.0], F32)))
    assert np.array_equal(bits(row), bits(nlms_params()))             # the restatement's own copy
    assert first_refused(table) is None


# ---- the library without a GPU --------------------------------------------------------------------------------------
def test_argument_checks_without_a_gpu():
    from gpuaudiobench_amd import _capi
    lib, bad = _capi.lib, _capi.GAB_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for args in ((0, 512, 64), (-1, 512, 64), (4, 0, 64), (4, -5, 64)):
        assert lib.gab_nlms_create(ctypes.byref(h), *args) == bad, args
        assert b"gab_nlms_create" in lib.gab_last_error() and not h.value
    for taps in (0, -64, 1, 32, 63, 65, 96, 192, 1024, 2 ** 30):
        assert lib.gab_nlms_create(ctypes.byref(h), 4, 512, taps) == bad, taps
        assert b"gab_nlms_create: taps must be 64, 128, 256 or 512" in lib.gab_last_error() and not h.value
    assert lib.gab_nlms_create(None, 4, 512, 64) == bad and b"null" in lib.gab_last_error()
    for call, name in ((lambda: lib.gab_nlms_process(None, None, None, None, None, None), b"gab_nlms_process"),
                       (lambda: lib.gab_nlms_process_batch(None, None, None, None, None, 1, None), b"gab_nlms_process_batch"),
                       (lambda: lib.gab_nlms_set_params(None, None, 1, None), b"gab_nlms_set_params"),
                       (lambda: lib.gab_nlms_set_params_tracks(None, None, 0, 1, 1, None), b"gab_nlms_set_params_tracks"),
                       (lambda: lib.gab_nlms_set_taps(None, None, None), b"gab_nlms_set_taps"),
                       (lambda: lib.gab_nlms_set_taps_tracks(None, None, 0, 1, None), b"gab_nlms_set_taps_tracks"),
                       (lambda: lib.gab_nlms_params(None, None, None, None), b"gab_nlms_params"),
                       (lambda: lib.gab_nlms_state(None, None, None, None), b"gab_nlms_state"),
                       (lambda: lib.gab_nlms_reset(None, None), b"gab_nlms_reset"),
                       (lambda: lib.gab_nlms_destroy(None), b"gab_nlms_destroy")):
        assert call() == bad
        assert name in lib.gab_last_error() and b"null pointer" in lib.gab_last_error()


def test_nlms_plan_is_exported():
    import gpuaudiobench_amd as g
    assert "NlmsPlan" in g.__all__ and "nlms_params" in g.__all__
    for name in ("set_params", "set_taps", "reset", "process", "process_batch", "params", "state", "prepare", "launch",
                 "close"):
        assert hasattr(g.NlmsPlan, name), name
    assert g.NlmsPlan.FIELDS == ("mu", "eps")
