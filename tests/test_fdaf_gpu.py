"""The fdaf plan (gab_fdaf_*) on the device.

Two kinds of comparison.  Bit for bit, device against device: every promise of the contract about what the bits do NOT
depend on (the cut into calls and batches, bufsize, alignment, in place, the other pairs, the shard, prepared and
captured calls), and the newest delay-line slot against the spectrum plan's row.  Against the float64 truth
(tests/fdaf_twin.py, wide), per pair: c = max |dev - truth| / (peak_a + peak_b), held to 4 times the same figure of the
complex64 restatement, the project's factor for a transform chain (tests/test_conv_levels_gpu.py).  Every figure is
printed before it is asserted.

Shapes: tracks {1, 2, 3, 5} (a lone odd track, one pair, a pair and an odd track, more than one wave), K {1, 2, 3, 4}
(no ring, a ring of a power of two and of three), bufsize {512, 1024, 1536}.  The streams and the truths are computed
once per scenario and shared, read only.
"""
import ctypes
import functools

import numpy as np
import pytest

from fdaf_twin import BINS, BLOCK, F32, FdafTwin, first_refused
from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_fdaf_host import CASES, EPS, decaying_taps, echo, erle_db, misalignment_db, noise, response, spoilt

pytestmark = pytest.mark.gpu

CENSUS = [(1, 1, 512), (2, 2, 1024), (3, 3, 1536), (5, 4, 512), (5, 2, 1536), (3, 1, 1024)]
MID = (5, 3, 1024)
# taps() of set_taps(h): two float32 transforms of 1024 points, each within about eps log2(N) = 6e-7 of the level
TAPS_BACK = 2e-6


def test_the_census_is_covered():
    assert {c[0] for c in CENSUS} == {1, 2, 3, 5} and {c[1] for c in CENSUS} == {1, 2, 3, 4}
    assert {c[2] for c in CENSUS} == {512, 1024, 1536}


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def state_of(plan):
    """(W, X as float32 [T][K][513][2], prev, count) on the host."""
    import torch
    w, x, pv, c = plan.state()
    return host(torch.view_as_real(w)), host(torch.view_as_real(x)), host(pv), host(c)


def same_state(a, b, rows=slice(None), rows_b=None):
    sa, sb = state_of(a), state_of(b)
    rows_b = rows if rows_b is None else rows_b
    return all(same(u[rows], v[rows_b]) for u, v in zip(sa[:3], sb[:3])) and np.array_equal(sa[3][rows], sb[3][rows_b])


def mix(T, seed):
    """Rows {mu, eps} that differ from track to track; every third track does not adapt."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.1, 0.6, T), np.exp(rng.uniform(np.log(1e-4), np.log(1e-1), T))], axis=1).astype(F32)
    p[(np.arange(T) + seed) % 3 == 2, 0] = 0.0
    return p


@functools.lru_cache(maxsize=None)
def stream(T, K, blocks, seed=0):
    """(p, taps, d, x): rows, starting taps and an echo under noise, [T][512 blocks]; read only."""
    x = noise(T, blocks * BLOCK, 100 + seed)
    d = noise(T, blocks * BLOCK, 200 + seed, 0.02)
    d[:, 5:] += F32(0.5) * x[:, :-5]
    out = (mix(T, 1 + seed), decaying_taps(T, K, 300 + seed), d, x)
    for a in out:
        a.setflags(write=False)
    return out


def buffers(a, B):
    """[T][n B] -> [n][T][B]"""
    T = a.shape[0]
    return np.ascontiguousarray(a.reshape(T, -1, B).transpose(1, 0, 2))


def started(gab, T, B, K, p=None, taps=None):
    plan = gab.FdafPlan(T, B, K)
    if p is not None:
        plan.set_params(dev(p))
    if taps is not None:
        plan.set_taps(dev(taps))
    return plan


def run(plan, d, x, err=True, est=True):
    """d, x [T][B] numpy -> (err, est) numpy [T][B], None where not asked for"""
    import torch
    n = plan.tracks * plan.bufsize
    e = torch.full((n,), 7.0, device="cuda") if err else None
    y = torch.full((n,), 7.0, device="cuda") if est else None
    plan.process(dev(d.ravel()), dev(x.ravel()), err=e, est=y)
    shape = (plan.tracks, plan.bufsize)
    return (host(e).reshape(shape) if err else None), (host(y).reshape(shape) if est else None)


def run_stream(plan, d, x):
    """The whole of d, x [T][n B] in single calls -> (err, est) [T][n B]"""
    outs = [run(plan, db, xb) for db, xb in zip(buffers(d, plan.bufsize), buffers(x, plan.bufsize))]
    return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)


# ---- 1. a new plan; the delay line against the spectrum plan ------------------------------------------------------
def test_a_new_plan_returns_the_input_and_plus_zero(gab):
    for T, K, B in ((3, 2, 1024), (2, 1, 512)):
        plan = gab.FdafPlan(T, B, K)
        assert (plan.tracks, plan.bufsize, plan.partitions) == (T, B, K)
        assert same(host(plan.params()), np.tile(np.array([0.0, 1.0], F32), (T, 1)))
        d, x = noise(T, B, 4, 1e3), noise(T, B, 5, 1e3)
        d[0, 3], d[1, 7], d[T - 1, 0] = -0.0, np.inf, np.nan
        e, y = run(plan, d, x)
        assert same(e, d) and not bits(y).any()
        W, X, pv, c = state_of(plan)
        assert not bits(W).any() and same(pv, x[:, -BLOCK:]) and (c == B // BLOCK).all()
        plan.close()


@pytest.mark.parametrize("T,K,B", CENSUS)
def test_the_newest_slot_is_the_spectrum_plans_row(gab, T, K, B):
    import torch
    p, taps, d, x = stream(T, K, 6)
    plan, spec = started(gab, T, B, K, p, taps), gab.SpectrumPlan(T, B, hop=512, mode="complex")
    spec.set_window(torch.ones(1024, device="cuda"))
    done = 0
    for db, xb in zip(buffers(d, B), buffers(x, B)):
        rows = host(spec.process(dev(xb.ravel())))                   # [B / 512][T][513][2], a frame per block
        run(plan, db, xb)
        done += B // BLOCK
        assert len(rows) == B // BLOCK
        X = state_of(plan)[1]
        for back in range(min(K, B // BLOCK)):                       # the frames of this buffer still in the ring
            assert same(X[:, (done - 1 - back) % K], rows[len(rows) - 1 - back]), (done, back)
    plan.close()
    spec.close()


# ---- 2. the cut -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,K,B", CENSUS)
def test_a_batch_is_its_single_launches(gab, T, K, B):
    import torch
    n = 4
    p, taps, d, x = stream(T, K, 12)
    d, x = d[:, :n * B], x[:, :n * B]
    a, b = started(gab, T, B, K, p, taps), started(gab, T, B, K, p, taps)
    se, sy = run_stream(a, d, x)
    e, y = torch.empty(n * T * B, device="cuda"), torch.empty(n * T * B, device="cuda")
    b.process_batch(dev(buffers(d, B).ravel()), dev(buffers(x, B).ravel()), err=e, est=y)
    assert same(buffers(se, B), host(e).reshape(n, T, B)) and same(buffers(sy, B), host(y).reshape(n, T, B))
    assert same_state(a, b) and (state_of(a)[3] == n * B // BLOCK).all()
    fresh = started(gab, T, B, K, p, taps)
    assert not same(state_of(a)[0], state_of(fresh)[0])               # the taps moved
    fresh.close()
    a.close()
    b.close()


@pytest.mark.parametrize("T,K", [(3, 2), (5, 3)])
def test_three_calls_at_512_are_one_at_1536(gab, T, K):
    p, taps, d, x = stream(T, K, 6)
    a, b = started(gab, T, 512, K, p, taps), started(gab, T, 1536, K, p, taps)
    (ea, ya), (eb, yb) = run_stream(a, d, x), run_stream(b, d, x)
    assert same(ea, eb) and same(ya, yb) and same_state(a, b)
    a.close()
    b.close()


# ---- 3. in place, one output, unaligned ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,K,B", [MID, (2, 1, 512)])
def test_in_place_one_output_and_unaligned(gab, T, K, B):
    import torch
    p, taps, d, x = stream(T, K, 6)
    n = d.shape[1] // B
    plans = [started(gab, T, B, K, p, taps) for _ in range(6)]
    ref, a, b, c, only_e, only_y = plans
    for db, xb in zip(buffers(d, B), buffers(x, B)):
        we, wy = run(ref, db, xb)
        dbuf, xbuf = dev(db.ravel()), dev(xb.ravel())
        e, y = a.process(dbuf, xbuf, err=dbuf, est=xbuf)              # err over d_in, est over d_ref
        assert e is dbuf and y is xbuf and same(host(dbuf).reshape(T, B), we) and same(host(xbuf).reshape(T, B), wy)
        off = [torch.full((T * B + 3,), 7.0, device="cuda") for _ in range(4)]
        off[0][1:T * B + 1] = dev(db.ravel())
        off[1][1:T * B + 1] = dev(xb.ravel())
        cut = [o[1:T * B + 1] for o in off]
        assert all(o.data_ptr() % 16 == 4 for o in cut)
        b.process(cut[0], cut[1], err=cut[2], est=cut[3])
        for o, want in ((off[2], we), (off[3], wy)):
            o = host(o)
            assert o[0] == 7.0 and (o[T * B + 1:] == 7.0).all() and same(o[1:T * B + 1].reshape(T, B), want)
        c.process(cut[0], cut[1], err=cut[0], est=cut[1])             # in place and unaligned
        assert same(host(cut[0]).reshape(T, B), we) and same(host(cut[1]).reshape(T, B), wy)
        e, y = run(only_e, db, xb, est=False)
        assert y is None and same(e, we)
        e, y = run(only_y, db, xb, err=False)
        assert e is None and same(y, wy)
        for q in plans[1:]:
            assert same_state(ref, q)
    assert n >= 2
    for q in plans:
        q.close()


# ---- 4. pairs -------------------------------------------------------------------------------------------------------
def test_a_shard_is_those_rows_of_the_whole(gab):
    T, K, B = MID
    p, taps, d, x = stream(T, K, 6)
    whole, shard = started(gab, T, B, K, p, taps), started(gab, 2, B, K, p[2:4], taps[2:4])
    (we, wy), (se, sy) = run_stream(whole, d, x), run_stream(shard, d[2:4], x[2:4])
    assert same(we[2:4], se) and same(wy[2:4], sy) and same_state(whole, shard, slice(2, 4), slice(0, 2))
    whole.close()
    shard.close()


def test_a_pair_is_a_function_of_its_own_pair(gab):
    T, K, B = MID
    p, taps, d, x = stream(T, K, 6)
    p2, taps2, d2, x2 = (np.array(a) for a in stream(T, K, 6, seed=9))
    for a, own in ((p2, p), (taps2, taps), (d2, d), (x2, x)):
        a[2:4] = own[2:4]
    one, other = started(gab, T, B, K, p, taps), started(gab, T, B, K, p2, taps2)
    (e1, y1), (e2, y2) = run_stream(one, d, x), run_stream(other, d2, x2)
    assert same(e1[2:4], e2[2:4]) and same(y1[2:4], y2[2:4]) and same_state(one, other, slice(2, 4))
    assert not same(e1[0:2], e2[0:2])
    one.close()
    other.close()


@pytest.mark.parametrize("K", [1, 3])
def test_an_odd_last_track_stands_beside_zeros(gab, K):
    """The contract's partner: zero samples, zero taps and the row {0, 1}."""
    B = 1024
    p, taps, d, x = (np.array(a) for a in stream(4, K, 6))
    p[0], p[2] = (0.5, 1e-3), (0.4, 1e-2)                            # both adapt
    for a, zero in ((p, (0.0, 1.0)), (taps, 0.0), (d, 0.0), (x, 0.0)):
        a[3] = zero
    odd, even = started(gab, 3, B, K, p[:3], taps[:3]), started(gab, 4, B, K, p, taps)
    (eo, yo), (ee, ye) = run_stream(odd, d[:3], x[:3]), run_stream(even, d, x)
    assert same(eo, ee[:3]) and same(yo, ye[:3]) and same_state(odd, even, slice(0, 3))
    assert not bits(state_of(even)[0][3]).any()
    odd.close()
    even.close()


# ---- 5. prepared and captured calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", [False, True])
def test_prepared_and_captured_calls_give_the_bits_of_plain_calls(gab, captured):
    import torch
    T, K, B = MID
    p, taps, ds, xs = stream(T, K, 6)
    plain, plan = started(gab, T, B, K, p, taps), started(gab, T, B, K, p, taps)
    we, wy = run_stream(plain, ds, xs)
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
        assert (state_of(plan)[3] == 0).all()                         # the capture recorded a launch without running it
    else:
        args = plan.prepare(d, x, err=e, est=y)
    for k, (db, xb) in enumerate(zip(buffers(ds, B), buffers(xs, B))):
        d.copy_(dev(db.ravel()))
        x.copy_(dev(xb.ravel()))
        if captured:
            graph.replay()
        else:
            plan.launch(args)
        torch.cuda.synchronize()
        cut = slice(k * B, (k + 1) * B)
        assert same(host(e).reshape(T, B), we[:, cut]) and same(host(y).reshape(T, B), wy[:, cut]), k
    assert same_state(plain, plan)
    if captured:
        del graph
    plain.close()
    plan.close()


# ---- 6. sets, a reset, a walk ----------------------------------------------------------------------------------------
def test_a_reset_is_a_new_plan_with_its_rows(gab):
    T, K, B = MID
    p, taps, d, x = stream(T, K, 6)
    used, new = started(gab, T, B, K, p, taps), started(gab, T, B, K, p)
    run_stream(used, d[:, :2 * B], x[:, :2 * B])
    used.reset()
    assert all(not bits(a).any() for a in state_of(used)[:3]) and not state_of(used)[3].any()
    assert same(host(used.params()), p)
    (e1, y1), (e2, y2) = run_stream(used, d, x), run_stream(new, d, x)
    assert same(e1, e2) and same(y1, y2) and same_state(used, new)
    used.close()
    new.close()


def walk(gab, batched, steps=30):
    """A seeded sequence of calls, sets and resets on one plan; every output and the final state."""
    import torch
    T, K, B = MID
    rng = np.random.default_rng(2025)
    plan = gab.FdafPlan(T, B, K)
    outs, tape = [], []
    for step in range(steps):
        kind = str(rng.choice(["process", "process", "batch", "batch", "params", "ranged", "taps", "ranged_taps",
                               "reset"])) if step else "params"
        tape.append(kind)
        if kind in ("params", "ranged"):
            lo = int(rng.integers(0, T - 1)) if kind == "ranged" else 0
            hi = int(rng.integers(lo + 1, T + 1)) if kind == "ranged" else T
            plan.set_params(dev(mix(T, 10 + step)[lo:hi]), first_track=lo if kind == "ranged" else None)
        elif kind in ("taps", "ranged_taps"):
            lo = int(rng.integers(0, T)) if kind == "ranged_taps" else 0
            h = decaying_taps(T, K, 50 + step)[lo:]
            plan.set_taps(dev(h), first_track=lo if kind == "ranged_taps" else None)
        elif kind == "reset":
            plan.reset()
        else:
            n = int(rng.integers(2, 4)) if kind == "batch" else 1
            d, x = buffers(noise(T, n * B, 1000 + step), B), buffers(noise(T, n * B, 2000 + step), B)
            if batched:
                e, y = plan.process_batch(dev(d.ravel()), dev(x.ravel()), err=torch.empty(n * T * B, device="cuda"),
                                          est=torch.empty(n * T * B, device="cuda"))
                outs.append((host(e).reshape(n, T, B), host(y).reshape(n, T, B)))
            else:
                each = [run(plan, d[i], x[i]) for i in range(n)]
                outs.append((np.stack([o[0] for o in each]), np.stack([o[1] for o in each])))
    assert {"process", "batch", "params", "ranged", "taps", "reset"} <= set(tape), tape
    return plan, outs


def test_a_seeded_walk_per_buffer_against_batched(gab):
    a, outs_a = walk(gab, False)
    b, outs_b = walk(gab, True)
    assert len(outs_a) == len(outs_b) >= 8
    for i, ((e1, y1), (e2, y2)) in enumerate(zip(outs_a, outs_b)):
        assert same(e1, e2) and same(y1, y2), i
    assert same_state(a, b) and same(host(a.params()), host(b.params()))
    a.close()
    b.close()


def test_sets_mid_stream_ranged_and_whole(gab):
    """A ranged set reaches its tracks' pairs and no other; set_taps leaves X, prev and count; the twin's taps."""
    T, K, B = MID
    p, taps, d, x = stream(T, K, 6)
    p2, taps2 = mix(T, 7), decaying_taps(T, K, 8)
    plan, still = started(gab, T, B, K, p, taps), started(gab, T, B, K, p, taps)
    for q in (plan, still):
        run_stream(q, d[:, :B], x[:, :B])
    plan.set_params(dev(p2[1:2]), first_track=1)
    plan.set_taps(dev(taps2[1:2]), first_track=1)
    got, kept = state_of(plan), state_of(still)
    assert all(same(u, v) for u, v in zip(got[1:3], kept[1:3])) and np.array_equal(got[3], kept[3])
    rest = np.array([0, 2, 3, 4])
    assert same(got[0][rest], kept[0][rest]) and not same(got[0][1], kept[0][1])
    want = p.copy()
    want[1] = p2[1]
    assert same(host(plan.params()), want)
    back = host(plan.taps())
    assert back.shape == (T, K * BLOCK) and np.abs(back[1] - taps2[1]).max() <= TAPS_BACK * np.abs(taps2[1]).max()
    (e1, y1), (e2, y2) = run_stream(plan, d[:, B:], x[:, B:]), run_stream(still, d[:, B:], x[:, B:])
    assert same(e1[2:], e2[2:]) and same(y1[2:], y2[2:]) and not same(y1[1], y2[1])
    plan.set_params(dev(p2))
    plan.set_taps(dev(taps2))
    assert same(host(plan.params()), p2) and np.abs(host(plan.taps()) - taps2).max() <= TAPS_BACK * np.abs(taps2).max()
    plan.close()
    still.close()


# ---- 7. against the float64 truth -----------------------------------------------------------------------------------
def pair_figures(got, truth):
    """c per pair: max |got - truth| / (peak_a + peak_b), the peaks the truth's; got, truth [T][n]."""
    T = truth.shape[0]
    out = []
    for q in range(0, T, 2):
        rows = slice(q, min(q + 2, T))
        out.append(np.abs(got[rows].astype(np.float64) - truth[rows]).max() / np.abs(truth[rows]).max(axis=1).sum())
    return np.array(out)


@functools.lru_cache(maxsize=None)
def truths(T, K, blocks, mu):
    """(p, taps, d, x, (err, est, taps) of the float32 restatement, the same of the float64 truth)"""
    taps = decaying_taps(T, K, 70)
    d, x, _ = echo(K, blocks, seed=50 + K, T=T)
    p = np.tile(np.array([mu, 1e-3], F32), (T, 1))
    outs = []
    for wide in (False, True):
        twin = FdafTwin(T, K, wide)
        twin.set_params(p)
        twin.set_taps(taps)
        outs.append(twin.process(d, x) + (twin.taps(),))
    return p, taps, d, x, outs[0], outs[1]


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_a_fixed_filter_is_within_4_c_twin_of_the_truth(gab, K):
    T, blocks = 3, 8
    p, taps, d, x, narrow, wide = truths(T, K, blocks, 0.0)
    plan = started(gab, T, 1024, K, p, taps)
    e, y = run_stream(plan, d, x)
    for name, got, n32, n64 in (("err", e, narrow[0], wide[0]), ("est", y, narrow[1], wide[1])):
        c_dev, c_twin = pair_figures(got, n64), pair_figures(n32, n64)
        print("fdaf mu=0 K=%d %s: c_dev %s c_twin %s ratio %s" % (K, name, c_dev, c_twin, c_dev / c_twin))
        assert (c_dev <= 4.0 * c_twin).all(), (name, c_dev, c_twin)
    plan.close()


# What feeds back through W.  err and est are held to the project's 4.  taps() exceeded it when it was measured; its
# bound is twice the largest factor on record (profiles/r32_fdaf.txt, DESIGN.md §4r, which also says why a feedback loop
# earns the margin).
ADAPTING_FACTOR = {"err": 4.0, "est": 4.0, "taps": 13.2}


@pytest.mark.parametrize("K", [2, 3, 4])
def test_an_adapting_filter_is_within_its_factor_of_the_truth(gab, K):
    """mu = 0.5, 16 blocks: err, est and taps().  (K = 1 at mu = 0.5 is no yardstick: tests/test_fdaf_host.py.)"""
    T, blocks = 3, 16
    p, taps, d, x, narrow, wide = truths(T, K, blocks, 0.5)
    plan = started(gab, T, 512, K, p, taps)
    e, y = run_stream(plan, d, x)
    back = host(plan.taps())
    for name, got, n32, n64 in (("err", e, narrow[0], wide[0]), ("est", y, narrow[1], wide[1]), ("taps", back, narrow[2], wide[2])):
        c_dev, c_twin = pair_figures(got, n64), pair_figures(n32, n64)
        print("fdaf adapting K=%d %s: c_dev %s c_twin %s ratio %s" % (K, name, c_dev, c_twin, c_dev / c_twin))
        assert (c_dev <= ADAPTING_FACTOR[name] * c_twin).all(), (name, c_dev, c_twin)
    plan.close()


@pytest.mark.parametrize("K", sorted(CASES))
def test_a_known_response_is_identified_on_the_device(gab, K):
    mu, blocks, condition, erle = CASES[K]
    d, x, h = echo(K, blocks)
    plan = started(gab, 1, 512, K, np.array([[mu, EPS]], F32))
    e = host(plan.process_batch(dev(d.ravel()), dev(x.ravel()))[0])
    mis = misalignment_db(host(plan.taps()), h)
    print("fdaf identification K=%d: misalignment %.1f dB, ERLE %.1f dB" % (K, mis, erle_db(d, e)))
    assert mis <= condition and np.array_equal(h, response(K))
    if erle is not None:
        assert erle_db(d, e) >= erle
    plan.close()


# ---- 8. containment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_what_is_not_finite_stays_in_its_pair_and_out_of_the_taps(gab, K):
    """tests/test_fdaf_host.py's streams plus a clean fifth track: K + 1 blocks of pair 0, one sample and one block of
    pair 1; the clean pairs are bit for bit a run without the bad samples, and W is finite throughout."""
    T, B, blocks = 5, 512, 10
    d4, x4, dirty_d4, dirty_x4, p4, skips = spoilt(4, K, blocks)
    extra_d, extra_x = noise(1, blocks * B, 90), noise(1, blocks * B, 91)
    d, x = np.concatenate([d4, extra_d]), np.concatenate([x4, extra_x])
    dirty_d, dirty_x = np.concatenate([dirty_d4, extra_d]), np.concatenate([dirty_x4, extra_x])
    p = np.concatenate([p4, p4[:1]])
    plan, clean = started(gab, T, B, K, p), started(gab, T, B, K, p)
    got_e, got_y = [], []
    for b in range(blocks):
        cut = slice(b * B, (b + 1) * B)
        e, y = run(plan, dirty_d[:, cut], dirty_x[:, cut])
        ce, cy = run(clean, d[:, cut], x[:, cut])
        assert same(e[4:], ce[4:]) and same(y[4:], cy[4:]) and same_state(plan, clean, slice(4, 5)), b
        W = state_of(plan)[0]
        assert np.isfinite(W).all(), b
        for pair in (0, 1):
            rows = slice(2 * pair, 2 * pair + 2)
            if b < min(skips[pair]):
                assert same(W[rows], state_of(clean)[0][rows]), (b, pair)
            elif b in skips[pair]:
                assert same(W[rows], before[rows]), (b, pair)         # the skipped block left W as it was
        before = W
        got_e.append(e), got_y.append(y)
    got_e, got_y = np.concatenate(got_e, axis=1), np.concatenate(got_y, axis=1)
    bad = np.zeros((T, blocks * B), bool)
    bad[0:2, 2 * B:(K + 3) * B] = True                               # the pair shares its transforms
    assert np.array_equal(~np.isfinite(got_y), bad)
    bad[3, 7 * B + 30] = True
    assert np.array_equal(~np.isfinite(got_e), bad)
    assert (state_of(plan)[3] == blocks).all()
    plan.close()
    clean.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    T, K, B = MID
    p, taps, d, x = stream(T, K, 6)
    plan, ref = started(gab, T, B, K, p, taps), started(gab, T, B, K, p, taps)
    up = lambda v, to=np.inf: np.nextafter(F32(v), F32(to))            # noqa: E731
    good = mix(T, 3)
    cases = [((2, 0), up(1.0, 2.0)), ((3, 0), np.nan), ((1, 0), np.inf), ((0, 0), -2.0 ** -149), ((2, 1), 0.0),
             ((3, 1), 2.0 ** -127), ((4, 1), up(2.0 ** 64)), ((0, 1), np.nan), ((1, 1), -1.0)]
    for (t, f), v in cases:
        bad = good.copy()
        bad[t, f] = v
        if t + 1 < T:
            bad[t + 1, 1] = np.nan                                    # the FIRST offender is named
        assert first_refused(bad) == 2 * t + f
        with pytest.raises(gab.GabError) as e:
            plan.set_params(dev(bad))
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
        assert "track %d field %d (%s)" % (t, f, ("mu", "eps")[f]) in str(e.value), str(e.value)
        assert "the plan keeps its parameters" in str(e.value)
    with pytest.raises(gab.GabError) as e:
        plan.set_params(dev(np.array([[0.5, 1.0], [1.5, 1.0]], F32)), first_track=3)
    assert "track 4 field 0 (mu) must be within [0, 1]" in str(e.value)
    h = np.zeros((2, K * BLOCK), F32)
    h[1, 700] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_taps(dev(h), first_track=2)
    assert "track 3 tap 700 must be finite; the plan keeps its taps" in str(e.value)
    edge = gab.FdafPlan(3, B, K)                                      # the edges themselves are admitted
    edge.set_params(dev(np.array([[-0.0, 2.0 ** -126], [1.0, 2.0 ** 64], [2.0 ** -149, 1.0]], F32)))
    edge.close()
    assert same(host(plan.params()), p) and same_state(plan, ref)
    (e1, y1), (e2, y2) = run_stream(plan, d[:, :B], x[:, :B]), run_stream(ref, d[:, :B], x[:, :B])
    assert same(e1, e2) and same(y1, y2)
    plan.close()
    ref.close()


def test_bad_arguments_leave_the_plan_usable(gab):
    T, K, B = MID
    p, taps, ds, xs = stream(T, K, 6)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    said = lambda text: text in lib.gab_last_error()                   # noqa: E731
    h = ctypes.c_void_p()
    create = lib.gab_fdaf_create
    for tracks, bufsize in ((0, 512), (4, 0), (-1, 512)):
        assert create(ctypes.byref(h), tracks, bufsize, 1) == bad and not h.value and said(b"tracks and bufsize must be > 0")
    for bufsize in (64, 256, 511, 513, 1000):
        assert create(ctypes.byref(h), 4, bufsize, 1) == bad and not h.value and said(b"bufsize must be a multiple of 512")
    for parts in (0, -1, 33):
        assert create(ctypes.byref(h), 4, 512, parts) == bad and not h.value and said(b"partitions must be 1..32")
    assert create(None, 4, 512, 1) == bad
    plan, ref = started(gab, T, B, K, p, taps), started(gab, T, B, K, p, taps)
    hp, n = plan._h, T * B
    big = dev(np.zeros(6 * n + 8, F32))
    at = lambda i: ctypes.c_void_p(big.data_ptr() + 4 * i)             # noqa: E731
    d, x, e, y = at(0), at(n), at(2 * n), at(3 * n)
    process = lib.gab_fdaf_process
    assert process(hp, None, x, e, y, None) == bad and said(b"null pointer")
    assert process(hp, d, None, e, y, None) == bad and said(b"null pointer")
    assert process(None, d, x, e, y, None) == bad and said(b"null pointer")
    assert process(hp, d, x, None, None, None) == bad and said(b"d_err and d_est may not both be null")
    assert process(hp, d, x, at(1), y, None) == bad and said(b"d_err may be d_in itself")
    assert process(hp, d, x, x, y, None) == bad and said(b"d_err may not overlap d_ref")
    assert process(hp, d, x, e, e, None) == bad and said(b"d_err may not overlap d_est")
    assert process(hp, d, x, None, at(n + 1), None) == bad and said(b"d_est may be d_ref itself")
    assert process(hp, d, x, e, d, None) == bad and said(b"d_est may not overlap d_in")
    batch = lib.gab_fdaf_process_batch
    assert batch(hp, d, x, e, y, 0, None) == bad and batch(hp, d, x, e, y, -3, None) == bad and said(b"n_buffers must be > 0")
    assert batch(hp, d, at(2 * n), at(4 * n - 1), None, 2, None) == bad and said(b"d_err may not overlap d_ref")
    assert batch(hp, d, x, e, y, (2 ** 31 - 1024) // B + 1, None) == bad and said(b"n_buffers * bufsize must be below 2^31 - 1024")
    pp = ctypes.c_void_p(dev(p).data_ptr())
    assert lib.gab_fdaf_set_params(hp, None, None) == bad and lib.gab_fdaf_set_taps(hp, None, None) == bad
    for first, cnt in ((-1, 2), (0, 0), (0, T + 1), (T, 1), (T - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_fdaf_set_params_tracks(hp, pp, first, cnt, None) == bad and said(b"the track range is outside the plan")
        assert lib.gab_fdaf_set_taps_tracks(hp, big.data_ptr(), first, cnt, None) == bad and said(b"outside the plan")
    assert lib.gab_fdaf_params(hp, None, None) == bad and lib.gab_fdaf_state(hp, None, None, None, None, None) == bad
    assert lib.gab_fdaf_reset(None, None) == bad and lib.gab_fdaf_destroy(None) == bad
    with pytest.raises(ValueError):
        plan.set_params(dev(p[:3]))
    with pytest.raises(ValueError):
        plan.set_taps(dev(np.zeros((T, K * BLOCK - 1), F32)))
    assert same_state(plan, ref) and same(host(plan.params()), p)
    (e1, y1), (e2, y2) = run_stream(plan, ds[:, :B], xs[:, :B]), run_stream(ref, ds[:, :B], xs[:, :B])
    assert same(e1, e2) and same(y1, y2) and same_state(plan, ref)
    plan.close()
    ref.close()
