"""The nlms plan (gab_nlms_*) on the device.

Every comparison is on bit patterns, of err, est, the taps and the history after every call, against NlmsTwin
(tests/nlms_twin.py): the contract fixes every rounding and the order of the tree, so the kernel has no freedom.  The
reference streams are computed once per scenario and shared, read only.

The kernel's cut (k_nlms.hip): a wave per track, four a workgroup, chunks of 64 samples, R = L / 64 registers of taps and
of window per lane.  CENSUS crosses every edge of it: a lone wave, a short last workgroup, more than one workgroup;
buffers below, at and above a chunk, one sample, odd sizes, buffers shorter than the history; every R.
"""
import ctypes
import functools

import numpy as np
import pytest

from nlms_twin import F32, NlmsTwin, not_finite
from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)

pytestmark = pytest.mark.gpu

TRACKS = (1, 3, 5, 9)
BUFSIZES = (1, 63, 64, 65, 100, 512)
TAPS = (64, 128, 256, 512)
# (tracks, bufsize, L): every value of each axis, and every L with a buffer below a chunk and one of at least a chunk
CENSUS = [(1, 1, 64), (3, 64, 64), (5, 63, 128), (9, 65, 128), (3, 1, 256), (1, 100, 256), (9, 63, 512), (5, 512, 512)]
MID = (5, 100, 128)                        # the shape of the scenarios below: a short last workgroup, B < L - 1


def test_the_census_is_covered():
    assert {c[0] for c in CENSUS} == set(TRACKS)
    assert {c[1] for c in CENSUS} == set(BUFSIZES)
    assert {(c[2], c[1] >= 64) for c in CENSUS} == {(L, big) for L in TAPS for big in (False, True)}


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def noise(T, n, seed, scale=0.25):
    return (scale * np.random.default_rng(seed).standard_normal((T, n))).astype(F32)


def signals(T, n, seed):
    """(d, x) [T][n]: the input holds an echo of the reference under noise of its own."""
    x = noise(T, n, seed)
    d = noise(T, n, seed + 1, 0.05)
    d[:, 3:] += F32(0.5) * x[:, :-3]
    return d, x


def nlms_mix(T, seed):
    """Rows {mu, eps} that differ from track to track; every third track does not adapt."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.05, 1.5, T), np.exp(rng.uniform(np.log(1e-8), np.log(1e-2), T))], axis=1).astype(F32)
    p[(np.arange(T) + seed) % 3 == 2, 0] = 0.0
    return p


def run(plan, d, x, err=True, est=True):
    """d, x [T][B] numpy -> (err, est) numpy, None where not asked for"""
    import torch
    n = plan.tracks * plan.bufsize
    e = torch.full((n,), 7.0, device="cuda") if err else None
    y = torch.full((n,), 7.0, device="cuda") if est else None
    plan.process(dev(d.ravel()), dev(x.ravel()), err=e, est=y)
    shape = (plan.tracks, plan.bufsize)
    return (host(e).reshape(shape) if err else None), (host(y).reshape(shape) if est else None)


def same_params(plan, cur, tgt):
    c, t = plan.params()
    return np.array_equal(bits(host(c)), bits(cur)) and np.array_equal(bits(host(t)), bits(tgt))


def state_is(plan, state):
    w, h = plan.state()
    return same(host(w), state[0]) and same(host(h), state[1])


def same_state(plan, twin):
    return state_is(plan, (twin.w, twin.hist))


@functools.lru_cache(maxsize=None)
def stream(T, B, L, n, ramp_at):
    """The shared scenario: nlms_mix(seed 1) at once, nlms_mix(seed 2) set with a ramp before buffer ramp_at, n buffers.
    Returns (p0, p1, ds [n][T][B], xs, errs, ests, the carried (taps, history) behind every buffer); read only."""
    p0, p1 = nlms_mix(T, 1), nlms_mix(T, 2)
    twin = NlmsTwin(T, B, L)
    twin.set_params(p0, ramp=False)
    d, x = signals(T, n * B, 100 + L + B)
    ds, xs = (a.reshape(T, n, B).transpose(1, 0, 2).copy() for a in (d, x))
    errs, ests, states = [], [], []
    for k in range(n):
        if k == ramp_at:
            twin.set_params(p1)
        e, y = twin.process(ds[k], xs[k])
        errs.append(e), ests.append(y), states.append((twin.w.copy(), twin.hist.copy()))
    errs, ests = np.stack(errs), np.stack(ests)
    for a in (p0, p1, ds, xs, errs, ests):
        a.setflags(write=False)
    return p0, p1, ds, xs, errs, ests, states


# ---- 1. the kernel against the contract -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,L", CENSUS)
def test_contract_bit_for_bit(gab, T, B, L):
    """Consecutive buffers: steady ones, a ramp buffer, steady ones behind it; the state crosses calls and chunk edges."""
    n = 3 if B >= 63 else 70
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, n, 1)
    plan = gab.NlmsPlan(T, B, L)
    assert (plan.tracks, plan.bufsize, plan.taps) == (T, B, L)
    plan.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == 1:
            plan.set_params(dev(p1))
            assert same_params(plan, p0, p1)
        e, y = run(plan, ds[k], xs[k])
        assert same(e, errs[k]) and same(y, ests[k]), k
        assert state_is(plan, states[k]), k
        if k == 1:
            assert same_params(plan, p1, p1)
    assert np.abs(states[-1][0]).max() > 1e-3                         # the taps moved
    plan.close()


def test_a_new_plan_returns_the_input_and_plus_zero(gab):
    for T, B, L in ((3, 70, 64), (9, 65, 512)):
        plan = gab.NlmsPlan(T, B, L)
        new = np.tile(np.array([0.0, 1.0], F32), (T, 1))
        assert same_params(plan, new, new)
        d, x = noise(T, B, 4, 1e3), noise(T, B, 5, 1e3)
        d[0, 3], d[1, 7], d[2, 0] = -0.0, np.inf, np.nan
        e, y = run(plan, d, x)
        assert same(e, d) and not bits(y).any()
        w, h = plan.state()
        assert not bits(host(w)).any() and same(host(h)[:, -min(B, L - 1):], x[:, -min(B, L - 1):])
        plan.close()


# ---- 2. batches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,L,n", [MID + (3,), (3, 1, 256, 70), (9, 65, 512, 2)])
@pytest.mark.parametrize("ramp_at", [None, 0])
def test_a_batch_is_its_single_launches(gab, T, B, L, n, ramp_at):
    """Steady, and with a ramp pending in front of the batch; a batch longer than L - 1 samples (300 against 127), one
    of 1-sample buffers, one shorter than the history (130 against 511)."""
    import torch
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, n + 1, ramp_at)
    a, b = gab.NlmsPlan(T, B, L), gab.NlmsPlan(T, B, L)
    for p in (a, b):
        p.set_params(dev(p0), ramp=False)
        if ramp_at == 0:
            p.set_params(dev(p1))
    singles = [run(a, ds[k], xs[k]) for k in range(n)]
    e, y = torch.empty(n * T * B, device="cuda"), torch.empty(n * T * B, device="cuda")
    b.process_batch(dev(ds[:n].ravel()), dev(xs[:n].ravel()), err=e, est=y)
    e, y = host(e).reshape(n, T, B), host(y).reshape(n, T, B)
    assert same(e, np.stack([s[0] for s in singles])) and same(y, np.stack([s[1] for s in singles]))
    assert same(e, errs[:n]) and same(y, ests[:n])
    assert state_is(a, states[n - 1]) and state_is(b, states[n - 1])
    last = p1 if ramp_at == 0 else p0
    assert same_params(a, last, last) and same_params(b, last, last)
    assert same(run(b, ds[n], xs[n])[0], errs[n])                     # and the stream goes on
    a.close()
    b.close()


# ---- 3. in place, one output, unaligned -------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,L", [MID, (9, 65, 128), (3, 64, 64)])
def test_in_place_one_output_and_unaligned(gab, T, B, L):
    import torch
    n = 3
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, n, 1)
    plans = [gab.NlmsPlan(T, B, L) for _ in range(5)]
    a, b, c, only_e, only_y = plans
    for p in plans:
        p.set_params(dev(p0), ramp=False)
    for k in range(n):
        if k == 1:
            for p in plans:
                p.set_params(dev(p1))
        dbuf, xbuf = dev(ds[k].ravel()), dev(xs[k].ravel())
        e, y = a.process(dbuf, xbuf, err=dbuf, est=xbuf)              # err over d_in, est over d_ref
        assert e is dbuf and y is xbuf
        assert same(host(dbuf).reshape(T, B), errs[k]) and same(host(xbuf).reshape(T, B), ests[k]), k
        # every block 4 bytes off a 16-byte boundary, guards around the outputs
        off = [torch.full((T * B + 3,), 7.0, device="cuda") for _ in range(4)]
        off[0][1:T * B + 1] = dev(ds[k].ravel())
        off[1][1:T * B + 1] = dev(xs[k].ravel())
        cut = [o[1:T * B + 1] for o in off]
        assert all(o.data_ptr() % 16 == 4 for o in cut)
        b.process(cut[0], cut[1], err=cut[2], est=cut[3])
        for o, want in ((off[2], errs[k]), (off[3], ests[k])):
            o = host(o)
            assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all() and same(o[1:T * B + 1].reshape(T, B), want), k
        c.process(cut[0], cut[1], err=cut[0], est=cut[1])             # in place and unaligned
        assert same(host(cut[0]).reshape(T, B), errs[k]) and same(host(cut[1]).reshape(T, B), ests[k]), k
        e, y = run(only_e, ds[k], xs[k], est=False)                   # either output null
        assert y is None and same(e, errs[k]), k
        e, y = run(only_y, ds[k], xs[k], err=False)
        assert e is None and same(y, ests[k]), k
        for p in plans:
            assert state_is(p, states[k]), k
    for p in plans:
        p.close()


# ---- 4. sets mid-stream -----------------------------------------------------------------------------------------
def test_sets_taps_and_reset_mid_stream(gab):
    """A ramped set, a set at once, a ranged set (the other rows' tables and bits untouched), set_taps on a range and on
    every track, a reset that drops a pending ramp."""
    T, B, L = MID
    n = 7
    p0, p1, p2 = nlms_mix(T, 1), nlms_mix(T, 2), nlms_mix(T, 3)
    d, x = signals(T, n * B, 50)
    plan, still, twin = gab.NlmsPlan(T, B, L), gab.NlmsPlan(T, B, L), NlmsTwin(T, B, L)
    for p in (plan, still):
        p.set_params(dev(p0), ramp=False)
    twin.set_params(p0, ramp=False)
    moved = np.zeros(T, bool)
    moved[1:3] = True
    taps = (0.1 * np.random.default_rng(9).standard_normal((T, L))).astype(F32)
    for k in range(n):
        if k == 1:
            plan.set_params(dev(p1))                                  # ramped
            twin.set_params(p1)
            still.set_params(dev(p1))
        if k == 2:
            for q in (p0[1:3], p2[1:3]):                              # ranged, twice before one buffer
                plan.set_params(dev(q), first_track=1)
                twin.set_params(q, first_track=1)
            cur, tgt = plan.params()
            assert np.array_equal(bits(host(cur)), bits(p1))
            assert np.array_equal(bits(host(tgt)[~moved]), bits(p1[~moved]))
            assert np.array_equal(bits(host(tgt)[moved]), bits(p2[moved]))
        if k == 3:
            plan.set_params(dev(p0[2:4]), ramp=False, first_track=2)  # at once
            twin.set_params(p0[2:4], first_track=2, ramp=False)
            plan.set_taps(dev(taps[1:3]), first_track=1)              # the history stays
            twin.set_taps(taps[1:3], first_track=1)
            assert same_state(plan, twin)
        if k == 4:
            plan.set_taps(dev(taps))
            twin.set_taps(taps)
            assert same_state(plan, twin)
        if k == 5:
            plan.set_params(dev(p2))                                  # pending: reset takes the target
            twin.set_params(p2)
            plan.reset()
            twin.reset()
            w, h = plan.state()
            assert not bits(host(w)).any() and not bits(host(h)).any() and same_params(plan, p2, p2)
        assert same_params(plan, twin.cur, twin.tgt), k
        dk, xk = d[:, k * B:(k + 1) * B], x[:, k * B:(k + 1) * B]
        (e, y), (es, _) = run(plan, dk, xk), run(still, dk, xk)
        we, wy = twin.process(dk, xk)
        assert same(e, we) and same(y, wy) and same_state(plan, twin), k
        assert same_params(plan, twin.cur, twin.tgt), k
        if k == 2:
            assert same(e[~moved], es[~moved]) and (bits(e[moved]) != bits(es[moved])).any()
    plan.close()
    still.close()


# ---- 5. a shard -------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, B, L = 9, 65, 128
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, 3, 1)
    lo, hi = 2, 7
    shard = gab.NlmsPlan(hi - lo, B, L)
    shard.set_params(dev(p0[lo:hi]), ramp=False)
    for k in range(3):
        if k == 1:
            shard.set_params(dev(p1[lo:hi]))
        e, y = run(shard, ds[k, lo:hi], xs[k, lo:hi])
        assert same(e, errs[k, lo:hi]) and same(y, ests[k, lo:hi]), k
        assert state_is(shard, (states[k][0][lo:hi], states[k][1][lo:hi])), k
    shard.close()


# ---- 6. prepared and captured calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("captured", [False, True])
def test_prepared_and_captured_calls_give_the_bits_of_plain_calls(gab, captured):
    import torch
    T, B, L = MID
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, 4, 0)
    plan = gab.NlmsPlan(T, B, L)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    e0, _ = run(plan, ds[0], xs[0])                                   # the ramp buffer, by a plain call: none pending
    assert same(e0, errs[0])
    d, x, e, y = (torch.zeros(T * B, device="cuda") for _ in range(4))
    if captured:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            args = plan.prepare(d, x, err=e, est=y)
            with torch.cuda.graph(graph, stream=side):
                plan.launch(args)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert state_is(plan, states[0])                              # the capture recorded a launch without running it
    else:
        args = plan.prepare(d, x, err=e, est=y)
    for k in range(1, 4):
        d.copy_(dev(ds[k].ravel()))
        x.copy_(dev(xs[k].ravel()))
        if captured:
            graph.replay()
        else:
            plan.launch(args)
        torch.cuda.synchronize()
        assert same(host(e).reshape(T, B), errs[k]) and same(host(y).reshape(T, B), ests[k]), k
        assert state_is(plan, states[k]), k
    if captured:
        del graph
    plan.close()


# ---- 7. a seeded walk of calls ----------------------------------------------------------------------------------
def test_a_seeded_walk_of_calls(gab):
    """About 40 calls on one plan, drawn from everything above, the twin beside it: state and outputs after every call."""
    import torch
    T, B, L = 5, 65, 128
    rng = np.random.default_rng(2024)
    plan, twin = gab.NlmsPlan(T, B, L), NlmsTwin(T, B, L)
    tape = []
    for step in range(40):
        kind = rng.choice(["process", "process", "in_place", "one_output", "batch", "batch", "params", "ranged", "taps",
                           "reset"]) if step else "params"
        tape.append(str(kind))
        if kind in ("params", "ranged"):
            lo = int(rng.integers(0, T - 1)) if kind == "ranged" else 0
            hi = int(rng.integers(lo + 1, T + 1)) if kind == "ranged" else T
            p, ramp = nlms_mix(T, 10 + step)[lo:hi], bool(rng.integers(0, 2))
            plan.set_params(dev(p), ramp=ramp, first_track=lo if kind == "ranged" else None)
            twin.set_params(p, ramp=ramp, first_track=lo)
        elif kind == "taps":
            lo = int(rng.integers(0, T))
            w = (0.05 * rng.standard_normal((T - lo, L))).astype(F32)
            plan.set_taps(dev(w), first_track=lo)
            twin.set_taps(w, first_track=lo)
        elif kind == "reset":
            plan.reset()
            twin.reset()
        else:
            n = int(rng.integers(1, 4)) if kind == "batch" else 1
            d, x = signals(T, n * B, 1000 + step)
            ds, xs = (a.reshape(T, n, B).transpose(1, 0, 2).copy() for a in (d, x))
            we, wy = twin.process_batch(ds, xs)
            dd, xd = dev(ds.ravel()), dev(xs.ravel())
            if kind == "batch":
                e, y = torch.empty_like(dd), torch.empty_like(dd)
                plan.process_batch(dd, xd, err=e, est=y)
            elif kind == "in_place":
                e, y = plan.process(dd, xd, err=dd, est=xd)
            elif kind == "one_output":
                e, y = plan.process(dd, xd, est=torch.empty_like(dd)) if step % 2 else plan.process(dd, xd)
            else:
                e, y = plan.process(dd, xd, err=torch.empty_like(dd), est=torch.empty_like(dd))
            assert e is None or same(host(e).reshape(n, T, B), we), (step, tape)
            assert y is None or same(host(y).reshape(n, T, B), wy), (step, tape)
        assert same_state(plan, twin) and same_params(plan, twin.cur, twin.tgt), (step, tape)
    assert {"process", "batch", "in_place", "params", "taps", "reset"} <= set(tape), tape
    plan.close()


# ---- 8. where float32 ends --------------------------------------------------------------------------------------
def test_what_is_not_finite_stays_in_its_track_and_out_of_the_taps(gab):
    """A NaN in x at sample 100 (L samples of err and est), an infinity in d (one sample of err); the clean neighbours
    are bit for bit a run without the bad tracks."""
    T, B, L, n = 5, 100, 64, 3
    p = np.tile(np.array([0.5, 1e-6], F32), (T, 1))
    d, x = signals(T, n * B, 60)
    dirty_d, dirty_x = d.copy(), x.copy()
    dirty_x[1, 100], dirty_d[3, 130] = np.nan, np.inf
    plan, clean, twin = gab.NlmsPlan(T, B, L), gab.NlmsPlan(T, B, L), NlmsTwin(T, B, L)
    for q in (plan, clean):
        q.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    want_bad = np.zeros((T, n * B), bool)
    want_bad[1, 100:100 + L] = True
    got_e, got_y = [], []
    for k in range(n):
        cut = slice(k * B, (k + 1) * B)
        e, y = run(plan, dirty_d[:, cut], dirty_x[:, cut])
        we, wy = twin.process(dirty_d[:, cut], dirty_x[:, cut])
        assert same(e, we) and same(y, wy) and same_state(plan, twin), k
        ce, cy = run(clean, d[:, cut], x[:, cut])
        ok = np.array([0, 2, 4])
        assert same(e[ok], ce[ok]) and same(y[ok], cy[ok]), k         # the neighbours never saw it
        w, h = plan.state()
        cw, ch = clean.state()
        assert not not_finite(host(w)).any() and same(host(w)[ok], host(cw)[ok]) and same(host(h)[ok], host(ch)[ok])
        got_e.append(e), got_y.append(y)
    got_e, got_y = np.concatenate(got_e, axis=1), np.concatenate(got_y, axis=1)
    assert np.array_equal(not_finite(got_y), want_bad)
    want_bad[3, 130] = True
    assert np.array_equal(not_finite(got_e), want_bad)
    assert twin.skipped == L + 1
    plan.close()
    clean.close()


def test_a_tail_through_the_subnormals(gab):
    from test_nlms_host import SUBNORMALS, subnormal_tail
    x, d, p = subnormal_tail()
    T, n = x.shape
    B = 64
    assert n % B == 0
    plan, twin = gab.NlmsPlan(T + 1, B, 64), NlmsTwin(T + 1, B, 64)
    x, d = np.concatenate([x, noise(1, n, 77)]), np.concatenate([d, noise(1, n, 78)])      # a loud neighbour
    p = np.concatenate([p, np.array([[0.5, 1e-6]], F32)])
    plan.set_params(dev(p), ramp=False)
    twin.set_params(p, ramp=False)
    es, ys = [], []
    for k in range(n // B):
        cut = slice(k * B, (k + 1) * B)
        e, y = run(plan, d[:, cut], x[:, cut])
        we, wy = twin.process(d[:, cut], x[:, cut])
        assert same(e, we) and same(y, wy) and same_state(plan, twin), k
        es.append(e[:T]), ys.append(y[:T])
    es, ys = np.concatenate(es, axis=1), np.concatenate(ys, axis=1)
    tiny = lambda a: int(((a != 0) & (np.abs(a) < 2.0 ** -126)).sum())             # noqa: E731
    assert (tiny(es), tiny(ys)) == SUBNORMALS[2:]                     # the device keeps its subnormals
    assert not not_finite(es).any() and not not_finite(ys).any()
    plan.close()


# ---- 9. identification ------------------------------------------------------------------------------------------
def test_a_known_response_is_identified_on_the_device(gab):
    """tests/test_nlms_host.py's case at L = 64 as eight 512-sample buffers: the twin's taps bit for bit, so its -80 dB."""
    from test_nlms_host import CASES, identified, response
    L, B = 64, 512
    n, mu = CASES[L]
    d, err, w, h = identified(L, False)
    x = (0.25 * np.random.default_rng(7).standard_normal(n)).astype(F32)
    plan = gab.NlmsPlan(1, B, L)
    plan.set_params(dev(np.array([[mu, 1e-6]], F32)), ramp=False)
    e = host(plan.process_batch(dev(d.ravel()), dev(x))[0])
    assert same(e, err.ravel())
    got = host(plan.state()[0])[0]
    assert same(got, w.astype(F32))
    mis = 10.0 * np.log10(((got.astype(np.float64) - h) ** 2).sum() / (h ** 2).sum())
    assert mis <= -80.0, mis
    assert np.array_equal(h, response(L))
    plan.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    from nlms_twin import first_refused
    T, B, L = MID
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, 3, 0)
    plan = gab.NlmsPlan(T, B, L)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    up = lambda v, to=np.inf: np.nextafter(F32(v), F32(to))            # noqa: E731
    good = nlms_mix(T, 3)
    cases = [((2, 0), up(2.0, 3.0)), ((3, 0), np.nan), ((1, 0), np.inf), ((0, 0), -2.0 ** -149), ((2, 1), 0.0),
             ((3, 1), 2.0 ** -127), ((4, 1), up(2.0 ** 64)), ((0, 1), np.nan), ((1, 1), -1.0)]
    for (t, f), v in cases:
        bad = good.copy()
        bad[t, f] = v
        if t + 1 < T:
            bad[t + 1, 1] = np.nan                                    # the FIRST offender is named
        assert first_refused(bad) == 2 * t + f
        for ramp in (True, False):
            with pytest.raises(gab.GabError) as e:
                plan.set_params(dev(bad), ramp=ramp)
            assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
            assert "track %d field %d (%s)" % (t, f, ("mu", "eps")[f]) in str(e.value), str(e.value)
            assert "the plan keeps its parameters" in str(e.value)
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(np.array([[0.5, 1.0], [2.5, 1.0]], F32)), first_track=3)
    assert "track 4 field 0" in str(e.value)
    w = np.zeros((2, L), F32)
    w[1, 7] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_taps(dev(w), first_track=2)
    assert "track 3 tap 7 must be finite; the plan keeps its taps" in str(e.value)
    edge = gab.NlmsPlan(3, B, L)                                      # the edges themselves are admitted
    edge.set_params(dev(np.array([[-0.0, 2.0 ** -126], [2.0, 2.0 ** 64], [2.0 ** -149, 1.0]], F32)))
    edge.close()
    assert same_params(plan, p0, p1)
    w0, _ = plan.state()
    assert not bits(host(w0)).any()
    for k in range(2):                                                # the pending ramp is still pending
        assert same(run(plan, ds[k], xs[k])[0], errs[k]), k
    plan.close()


def test_bad_arguments_leave_the_plan_usable(gab):
    T, B, L = MID
    p0, p1, ds, xs, errs, ests, states = stream(T, B, L, 3, 0)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    said = lambda text: text in lib.gab_last_error()                   # noqa: E731
    h = ctypes.c_void_p()
    for taps in (0, 32, 96, 1024):
        assert lib.gab_nlms_create(ctypes.byref(h), 4, 64, taps) == bad and not h.value, taps
        assert said(b"taps must be 64, 128, 256 or 512")
    with pytest.raises(gab.GabError):
        gab.NlmsPlan(4, 64, 100)
    plan = gab.NlmsPlan(T, B, L)
    plan.set_params(dev(p0), ramp=False)
    plan.set_params(dev(p1))
    hp, n = plan._h, T * B
    big = dev(np.zeros(6 * n + 8, F32))
    at = lambda i: ctypes.c_void_p(big.data_ptr() + 4 * i)             # noqa: E731
    d, x, e, y = at(0), at(n), at(2 * n), at(3 * n)
    process = lib.gab_nlms_process
    assert process(hp, None, x, e, y, None) == bad and said(b"null pointer")
    assert process(hp, d, None, e, y, None) == bad and said(b"null pointer")
    assert process(None, d, x, e, y, None) == bad and said(b"null pointer")
    assert process(hp, d, x, None, None, None) == bad and said(b"d_err and d_est may not both be null")
    assert process(hp, d, x, at(1), y, None) == bad and said(b"d_err may be d_in itself")          # a partial overlap
    assert process(hp, d, x, at(n - 1), y, None) == bad and said(b"d_err may be d_in itself")
    assert process(hp, d, x, x, y, None) == bad and said(b"d_err may not overlap d_ref")
    assert process(hp, d, x, at(2 * n - 1), y, None) == bad and said(b"d_err may not overlap d_ref")
    assert process(hp, d, x, e, e, None) == bad and said(b"d_err may not overlap d_est")
    assert process(hp, d, x, e, at(3 * n - 1), None) == bad and said(b"d_err may not overlap d_est")
    assert process(hp, d, x, None, at(n + 1), None) == bad and said(b"d_est may be d_ref itself")
    assert process(hp, d, x, e, d, None) == bad and said(b"d_est may not overlap d_in")
    assert process(hp, d, at(4 * n), None, at(1), None) == bad and said(b"d_est may not overlap d_in")
    batch = lib.gab_nlms_process_batch
    assert batch(hp, d, x, e, y, 0, None) == bad and batch(hp, d, x, e, y, -3, None) == bad and said(b"n_buffers")
    assert batch(hp, d, at(2 * n), at(4 * n - 1), None, 2, None) == bad and said(b"d_err may not overlap d_ref")   # two buffers long
    pp = ctypes.c_void_p(dev(p0).data_ptr())
    assert lib.gab_nlms_set_params(hp, None, 1, None) == bad and lib.gab_nlms_set_taps(hp, None, None) == bad
    for first, cnt in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_nlms_set_params_tracks(hp, pp, first, cnt, 1, None) == bad and said(b"outside the plan"), (first, cnt)
        assert lib.gab_nlms_set_taps_tracks(hp, big.data_ptr(), first, cnt, None) == bad and said(b"outside the plan")
    assert lib.gab_nlms_params(hp, None, None, None) == bad and lib.gab_nlms_state(hp, None, None, None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p0.ravel()[:3]))
    with pytest.raises(ValueError):
        plan.set_params(dev(p0[:3]))
    with pytest.raises(ValueError):
        plan.set_taps(dev(np.zeros((T, L - 1), F32)))
    assert same_params(plan, p0, p1)
    for k in range(2):                                                # nothing moved: the stream is the scenario's
        e, y = run(plan, ds[k], xs[k])
        assert same(e, errs[k]) and same(y, ests[k]) and state_is(plan, states[k]), k
    plan.close()
