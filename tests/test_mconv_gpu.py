"""The matrix-convolution plan (gab_mconv_*) on the device.

Two kinds of comparison.  Bit for bit, device against device: a diagonal table against the fdaf plan's estimate, the
newest ring slot against the spectrum plan's row, and every promise of the contract about what the bits do NOT depend
on (the cut into calls, batches and rounds, bufsize, alignment, the shard of outputs, prepared and captured calls), the
sets and the ramp.  Against the float64 truth (tests/mconv_twin.py, wide), per pair of outputs: c = max |dev - truth| /
(peak_a + peak_b), held to 4 times the same figure of the complex64 restatement, the project's factor for a transform
chain (tests/test_conv_levels_gpu.py).  Every figure is printed before it is asserted.

Shapes: inputs {1, 2, 3, 5, 33, 65} (a lone odd input, a pair, more than one wave, one and two group cuts), outputs
{1, 2, 3}, K {1, 2, 3}, bufsize {512, 1024, 1536}.  The streams and the truths are computed once and shared, read only.
"""
import ctypes
import functools

import numpy as np
import pytest

from mconv_twin import BINS, BLOCK, F32, MconvTwin
from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)
from test_mconv_host import decaying_taps, noise
from test_mix_host import fma32

pytestmark = pytest.mark.gpu

CENSUS = [(1, 1, 1, 512), (2, 2, 2, 1024), (3, 3, 3, 1536), (5, 2, 1, 1024), (33, 3, 2, 512), (65, 1, 3, 512)]   # (I, O, K, B)
MID = (5, 3, 2, 1024)


def test_the_census_is_covered():
    assert {c[0] for c in CENSUS} == {1, 2, 3, 5, 33, 65} and {c[1] for c in CENSUS} == {1, 2, 3}
    assert {c[2] for c in CENSUS} == {1, 2, 3} and {c[3] for c in CENSUS} == {512, 1024, 1536}


def same(a, b):
    """Bit for bit; where both hold a NaN the payload is not compared."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


def state_of(plan):
    """(H_current, H_target, X as float32 [...][513][2], prev, count) on the host."""
    import torch
    hc, ht, x, pv, c = plan.state()
    return host(torch.view_as_real(hc)), host(torch.view_as_real(ht)), host(torch.view_as_real(x)), host(pv), c


def same_state(a, b):
    sa, sb = state_of(a), state_of(b)
    return all(same(u, v) for u, v in zip(sa[:4], sb[:4])) and sa[4] == sb[4]


@functools.lru_cache(maxsize=None)
def stream(I, O, K, blocks, seed=0):
    """(taps [O][I][512 K], x [I][512 blocks]); read only."""
    out = (decaying_taps(O, I, K, 300 + seed), noise(I, blocks * BLOCK, 100 + seed))
    for a in out:
        a.setflags(write=False)
    return out


def buffers(a, B):
    """[T][n B] -> [n][T][B]"""
    T = a.shape[0]
    return np.ascontiguousarray(a.reshape(T, -1, B).transpose(1, 0, 2))


def started(gab, I, O, B, K, taps=None):
    plan = gab.MatrixConvPlan(I, O, B, K)
    if taps is not None:
        plan.set_taps(dev(taps), ramp=False)
    return plan


def run(plan, x):
    """x [I][B] numpy -> [O][B]"""
    import torch
    y = torch.full((plan.outputs * plan.bufsize,), 7.0, device="cuda")
    plan.process(dev(x.ravel()), out=y)
    return host(y).reshape(plan.outputs, plan.bufsize)


def run_stream(plan, x):
    """The whole of x [I][n B] in single calls -> [O][n B]"""
    return np.concatenate([run(plan, xb) for xb in buffers(x, plan.bufsize)], axis=1)


def run_batch(plan, x):
    """The whole of x [I][n B] in one batch -> [O][n B]"""
    n = x.shape[1] // plan.bufsize
    y = host(plan.process_batch(dev(buffers(x, plan.bufsize).ravel()))).reshape(n, plan.outputs, plan.bufsize)
    return y.transpose(1, 0, 2).reshape(plan.outputs, -1)


# ---- (a) a new plan; (b) the fdaf plan; (c) the spectrum plan -------------------------------------------------------
def test_a_new_plan_gives_plus_zero(gab):
    for I, O, K, B in ((3, 3, 2, 1024), (2, 1, 1, 512), (33, 2, 1, 512)):
        plan = gab.MatrixConvPlan(I, O, B, K)
        assert (plan.inputs, plan.outputs, plan.bufsize, plan.partitions) == (I, O, B, K)
        x = noise(I, B, 4, 1e3)
        x[0, 3] = -0.0
        assert not bits(run(plan, x)).any()
        hc, ht, X, pv, c = state_of(plan)
        assert not bits(hc).any() and not bits(ht).any() and same(pv, x[:, -BLOCK:]) and c == B // BLOCK
        assert X.shape == (K + 15, I, BINS, 2) and hc.shape == (O, I, K, BINS, 2)
        plan.close()


@pytest.mark.parametrize("n,K", [(n, K) for n in (1, 2, 3, 5) for K in (1, 2, 3)] + [(34, 2)])
def test_a_diagonal_table_is_the_fdaf_plans_estimate(gab, n, K):
    """The pairings, transforms, products and the last fmaf are the same, and a product with a zero spectrum adds a zero."""
    import torch
    B = 1024
    taps, x = stream(n, 1, K, 6, seed=n)
    table = np.zeros((n, n, K * BLOCK), F32)
    table[np.arange(n), np.arange(n)] = taps[0]
    plan, fdaf = started(gab, n, n, B, K, table), gab.FdafPlan(n, B, K)
    fdaf.set_taps(dev(taps[0]))
    for k, xb in enumerate(buffers(x, B)):
        est = torch.empty(n * B, device="cuda")
        fdaf.process(dev(np.zeros_like(xb).ravel()), dev(xb.ravel()), est=est)
        y = run(plan, xb)
        assert same(y, host(est).reshape(n, B)), k
        assert np.abs(y).max() > 0
    plan.close()
    fdaf.close()


@pytest.mark.parametrize("I,O,K,B", CENSUS)
def test_the_newest_slot_is_the_spectrum_plans_row(gab, I, O, K, B):
    import torch
    taps, x = stream(I, O, K, 6)
    plan, spec = started(gab, I, O, B, K, taps), gab.SpectrumPlan(I, B, hop=512, mode="complex")
    spec.set_window(torch.ones(1024, device="cuda"))
    done, S = 0, K + 15
    for xb in buffers(x, B):
        rows = host(spec.process(dev(xb.ravel())))                   # [B / 512][I][513][2], a frame per block
        run(plan, xb)
        done += B // BLOCK
        assert len(rows) == B // BLOCK
        X = state_of(plan)[2]
        for back in range(B // BLOCK):
            assert same(X[(done - 1 - back) % S], rows[len(rows) - 1 - back]), (done, back)
    plan.close()
    spec.close()


# ---- (d) the cut; (e) alignment ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,O,K,B", CENSUS)
def test_a_batch_is_its_single_calls(gab, I, O, K, B):
    taps, x = stream(I, O, K, 12)
    x = x[:, :4 * B]
    a, b = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    assert same(run_stream(a, x), run_batch(b, x)) and same_state(a, b) and state_of(a)[4] == 4 * B // BLOCK
    a.close()
    b.close()


@pytest.mark.parametrize("I,O,K", [(3, 2, 2), (33, 3, 3)])
def test_three_calls_at_512_are_one_at_1536(gab, I, O, K):
    taps, x = stream(I, O, K, 6)
    a, b = started(gab, I, O, 512, K, taps), started(gab, I, O, 1536, K, taps)
    assert same(run_stream(a, x), run_stream(b, x)) and same_state(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("I,O,K,B,n", [(3, 3, 3, 512, 19), (5, 2, 2, 1536, 12), (65, 1, 1, 512, 33)])
def test_a_call_of_more_than_one_round_is_its_single_blocks(gab, I, O, K, B, n):
    """17 blocks and more: several rounds of the launches, the ring turning over under them."""
    taps, x = stream(I, O, K, n * B // BLOCK, seed=2)
    a, b = started(gab, I, O, 512, K, taps), started(gab, I, O, B, K, taps)
    assert n * B // BLOCK >= 17 and same(run_stream(a, x), run_batch(b, x)) and same_state(a, b)
    a.close()
    b.close()


def test_four_bytes_off_alignment(gab):
    import torch
    I, O, K, B = MID
    taps, x = stream(I, O, K, 6)
    ref, plan = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    for xb in buffers(x, B):
        want = run(ref, xb)
        src, dst = torch.full((I * B + 3,), 7.0, device="cuda"), torch.full((O * B + 3,), 7.0, device="cuda")
        src[1:I * B + 1] = dev(xb.ravel())
        assert src[1:].data_ptr() % 16 == 4 and dst[1:].data_ptr() % 16 == 4
        plan.process(src[1:I * B + 1], out=dst[1:O * B + 1])
        got = host(dst)
        assert got[0] == 7.0 and (got[O * B + 1:] == 7.0).all() and same(got[1:O * B + 1].reshape(O, B), want)
    assert same_state(ref, plan)
    ref.close()
    plan.close()


# ---- (f) a shard of outputs; (g) a group alone ------------------------------------------------------------------------
@pytest.mark.parametrize("O,lo,n", [(3, 2, 1), (4, 2, 2), (3, 0, 2)])
def test_an_output_shard_from_an_even_output_is_those_rows(gab, O, lo, n):
    I, K, B = 5, 2, 1024
    taps, x = stream(I, O, K, 6)
    whole, shard = started(gab, I, O, B, K, taps), started(gab, I, n, B, K, taps[lo:lo + n])
    assert same(run_stream(whole, x)[lo:lo + n], run_stream(shard, x))
    sw, ss = state_of(whole), state_of(shard)
    assert same(sw[1][lo:lo + n], ss[1]) and same(sw[2], ss[2]) and same(sw[3], ss[3])
    whole.close()
    shard.close()


def test_group_1_alone_is_a_plan_of_its_32_inputs(gab):
    I, O, K, B = 65, 2, 2, 512
    taps, x = stream(I, O, K, 5)
    fed = np.zeros_like(x)
    fed[32:64] = x[32:64]
    whole, part = started(gab, I, O, B, K, taps), started(gab, 32, O, B, K, taps[:, 32:64])
    y = run_stream(whole, fed)
    assert same(y, run_stream(part, x[32:64])) and np.abs(y).max() > 0
    whole.close()
    part.close()


# ---- (h), (i), (j) sets; (k) a reset ----------------------------------------------------------------------------------
@pytest.mark.parametrize("I,O,K,B", [MID, (33, 2, 3, 512)])
def test_an_unramped_set_mid_stream_is_the_plan_that_had_the_taps(gab, I, O, K, B):
    taps, x = stream(I, O, K, 6 * B // BLOCK)
    taps2 = decaying_taps(O, I, K, 77)
    moved, there = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps2)
    for k, xb in enumerate(buffers(x, B)):
        if k == 2:
            moved.set_taps(dev(taps2), ramp=False)
        assert same(run(moved, xb), run(there, xb)) == (k >= 2), k
    assert same_state(moved, there)
    moved.close()
    there.close()


@pytest.mark.parametrize("I,O,K,B,batched", [MID + (False,), (33, 3, 1, 1536, False), (5, 3, 2, 1024, True)])
def test_a_ramped_set_is_the_fmaf_blend_of_the_two_plans(gab, I, O, K, B, batched):
    taps, x = stream(I, O, K, 6 * B // BLOCK)
    taps2 = decaying_taps(O, I, K, 78)
    moved, old, new = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps2)
    r = ((np.arange(B, dtype=np.float64) + 1.0) / B).astype(F32)
    bufs = buffers(x, B)
    ya, yb = run_stream(old, x), run_stream(new, x)
    want = np.concatenate([ya[:, :2 * B], fma32(yb[:, 2 * B:3 * B] - ya[:, 2 * B:3 * B], r[None, :], ya[:, 2 * B:3 * B]),
                           yb[:, 3 * B:]], axis=1)
    got = [run(moved, bufs[0]), run(moved, bufs[1])]
    moved.set_taps(dev(taps2), ramp=True)
    hc, ht = state_of(moved)[:2]
    assert same(hc, state_of(old)[0]) and same(ht, state_of(new)[1])
    if batched:                                                       # the first buffer of a batch takes the ramp
        got.append(run_batch(moved, x[:, 2 * B:]))
    else:
        got += [run(moved, b) for b in bufs[2:]]
    got = np.concatenate(got, axis=1)
    for k in range(6):
        assert same(got[:, k * B:(k + 1) * B], want[:, k * B:(k + 1) * B]), k
    assert not same(got[:, 2 * B:3 * B], ya[:, 2 * B:3 * B]) and not same(got[:, 2 * B:3 * B], yb[:, 2 * B:3 * B])
    assert same_state(moved, new)
    for q in (moved, old, new):
        q.close()


def test_a_ranged_set_is_the_whole_set_of_the_merged_table(gab):
    I, O, K, B = 33, 3, 2, 512
    taps, x = stream(I, O, K, 4)
    taps2 = decaying_taps(O, I, K, 79)
    merged = taps.copy()
    merged[1:3, 30:33] = taps2[1:3, 30:33]
    merged[0:1, 0:2] = taps2[0:1, 0:2]
    a, b = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, merged)
    a.set_taps(dev(taps2[1:3, 30:33]), ramp=False, first_output=1, first_input=30)
    a.set_taps(dev(taps2[0:1, 0:2]), ramp=False, first_output=0)
    assert same_state(a, b) and same(run_stream(a, x), run_stream(b, x))
    a.close()
    b.close()


def test_a_reset_is_a_new_plan_with_its_taps(gab):
    I, O, K, B = MID
    taps, x = stream(I, O, K, 6 * B // BLOCK)
    taps2 = decaying_taps(O, I, K, 80)
    used, new = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps2)
    run_stream(used, x[:, :2 * B])
    used.set_taps(dev(taps2), ramp=True)
    used.reset()                                                      # the ramp is dropped: current := target
    s = state_of(used)
    assert not bits(s[2]).any() and not bits(s[3]).any() and s[4] == 0 and same(s[0], s[1])
    assert same(run_stream(used, x), run_stream(new, x)) and same_state(used, new)
    used.close()
    new.close()


# ---- (l) prepared and captured calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("captured", [False, True])
def test_prepared_and_captured_calls_give_the_bits_of_plain_calls(gab, captured):
    """Steady: no ramp is pending at the capture (the header's "Captured calls")."""
    import torch
    I, O, K, B = MID
    taps, xs = stream(I, O, K, 6 * B // BLOCK)
    plain, plan = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    want = run_stream(plain, xs)
    x, y = torch.zeros(I * B, device="cuda"), torch.zeros(O * B, device="cuda")
    if captured:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            args = plan.prepare(x, y)
            with torch.cuda.graph(graph, stream=side):
                plan.launch(args)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert state_of(plan)[4] == 0                                 # the capture recorded the launches without running them
    else:
        args = plan.prepare(x, y)
    for k, xb in enumerate(buffers(xs, B)):
        x.copy_(dev(xb.ravel()))
        if captured:
            graph.replay()
        else:
            plan.launch(args)
        torch.cuda.synchronize()
        assert same(host(y).reshape(O, B), want[:, k * B:(k + 1) * B]), k
    assert same_state(plain, plan)
    if captured:
        del graph
    plain.close()
    plan.close()


# ---- (m) containment ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
def test_what_is_not_finite_leaves_after_k_plus_1_blocks_and_never_reaches_the_taps(gab, K):
    I, O, B, blocks = 3, 3, 512, K + 6
    taps, x = (np.array(a) for a in stream(I, O, K, blocks))
    taps[1, 0] = 0.0                                                  # NaN 0 is NaN: output 1 is not spared
    dirty, zeroed = x.copy(), x.copy()
    dirty[0, 2 * B + 5], dirty[0, 2 * B + 300] = np.nan, np.inf
    zeroed[0, 2 * B + 5] = zeroed[0, 2 * B + 300] = 0.0
    plan, clean = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    H = state_of(plan)[:2]
    for b in range(blocks):
        y, want = run(plan, dirty[:, b * B:(b + 1) * B]), run(clean, zeroed[:, b * B:(b + 1) * B])
        bad = 2 <= b < 2 + K + 1                                      # the sample lies in two windows
        assert (~np.isfinite(y)).all() == bad and np.isfinite(y).all() == (not bad), b
        if not bad:
            assert same(y, want), b
        now = state_of(plan)[:2]
        assert same(now[0], H[0]) and same(now[1], H[1]), b
    plan.close()
    clean.close()


# ---- (n) refusals -------------------------------------------------------------------------------------------------------
def test_a_refused_table_changes_nothing(gab):
    I, O, K, B = MID
    taps, x = stream(I, O, K, 2)
    plan, ref = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    h = np.zeros((2, 2, K * BLOCK), F32)
    h[1, 0, 700], h[1, 1, 3] = np.inf, np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_taps(dev(h), ramp=True, first_output=1, first_input=3)
    assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
    assert "output 2 input 3 tap 700 must be finite; the plan keeps its taps" in str(e.value)
    whole = np.array(taps)
    whole[2, 4, K * BLOCK - 1] = np.nan
    with pytest.raises(gab.GabError) as e:
        plan.set_taps(dev(whole), ramp=False)
    assert "output 2 input 4 tap %d must be finite" % (K * BLOCK - 1) in str(e.value)
    assert same_state(plan, ref) and same(run_stream(plan, x[:, :B]), run_stream(ref, x[:, :B]))    # and no ramp is pending
    assert same_state(plan, ref)
    plan.close()
    ref.close()


def test_bad_arguments_leave_the_plan_usable(gab):
    I, O, K, B = MID
    taps, xs = stream(I, O, K, 2)
    lib, bad = gab.lib, gab._capi.GAB_ERR_INVALID_ARG
    said = lambda text: text in lib.gab_last_error()                   # noqa: E731
    h = ctypes.c_void_p()
    create = lib.gab_mconv_create
    for inputs, bufsize in ((0, 512), (4, 0), (-1, 512)):
        assert create(ctypes.byref(h), inputs, bufsize, 2, 1) == bad and not h.value and said(b"tracks and bufsize must be > 0")
    assert create(ctypes.byref(h), 4097, 512, 1, 1) == bad and not h.value and said(b"inputs must be 1..4096")
    for outputs in (0, -1, 65):
        assert create(ctypes.byref(h), 4, 512, outputs, 1) == bad and not h.value and said(b"outputs must be 1..64")
    for parts in (0, -1, 33):
        assert create(ctypes.byref(h), 4, 512, 2, parts) == bad and not h.value and said(b"partitions must be 1..32")
    for shape in ((4096, 17, 1), (1025, 64, 1), (64, 64, 17)):
        assert create(ctypes.byref(h), shape[0], 512, shape[1], shape[2]) == bad and not h.value
        assert said(b"inputs * outputs * partitions must be at most 65536")
    for bufsize in (64, 256, 511, 513, 1000):
        assert create(ctypes.byref(h), 4, bufsize, 2, 1) == bad and not h.value and said(b"bufsize must be a multiple of 512")
    assert create(None, 4, 512, 2, 1) == bad
    plan, ref = started(gab, I, O, B, K, taps), started(gab, I, O, B, K, taps)
    hp, n_in, n_out = plan._h, I * B, O * B
    big = dev(np.zeros(3 * (n_in + n_out) + 8, F32))
    at = lambda i: ctypes.c_void_p(big.data_ptr() + 4 * i)             # noqa: E731
    x, y = at(0), at(2 * n_in)
    process, batch = lib.gab_mconv_process, lib.gab_mconv_process_batch
    assert process(hp, None, y, None) == bad and said(b"null pointer")
    assert process(hp, x, None, None) == bad and said(b"null pointer")
    assert process(None, x, y, None) == bad and said(b"null pointer")
    for out in (x, at(n_in - 1), at(1)):
        assert process(hp, x, out, None) == bad and said(b"d_out may not overlap d_in")
    assert process(hp, at(n_out), at(1), None) == bad and said(b"d_out may not overlap d_in")      # d_out in front, its tail inside
    assert batch(hp, x, y, 0, None) == bad and batch(hp, x, y, -3, None) == bad and said(b"n_buffers must be > 0")
    assert batch(hp, x, at(2 * n_in - 1), 2, None) == bad and said(b"d_out may not overlap d_in")
    assert batch(hp, x, y, (2 ** 31 - 1024) // B + 1, None) == bad and said(b"n_buffers * bufsize must be below 2^31 - 1024")
    assert lib.gab_mconv_set_taps(hp, None, 0, None) == bad and said(b"null pointer")
    assert lib.gab_mconv_set_taps_range(hp, None, 0, 1, 0, 1, 0, None) == bad and said(b"null pointer")
    t = big.data_ptr()
    for first, cnt in ((-1, 2), (0, 0), (0, I + 1), (I, 1), (I - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_mconv_set_taps_range(hp, t, 0, 1, first, cnt, 0, None) == bad and said(b"the track range is outside the plan")
    for first, cnt in ((-1, 2), (0, 0), (0, O + 1), (O, 1), (O - 1, 2), (2 ** 31 - 1, 2)):
        assert lib.gab_mconv_set_taps_range(hp, t, first, cnt, 0, 1, 1, None) == bad and said(b"the output range is outside the plan")
    assert lib.gab_mconv_state(hp, None, None, None, None, None, None) == bad
    assert lib.gab_mconv_reset(None, None) == bad and lib.gab_mconv_destroy(None) == bad
    with pytest.raises(ValueError):
        plan.set_taps(dev(np.zeros((O, I, K * BLOCK - 1), F32)))
    with pytest.raises(ValueError):
        plan.set_taps(dev(np.zeros((O * I * K * BLOCK,), F32)), first_output=0)
    assert same_state(plan, ref) and same(run_stream(plan, xs), run_stream(ref, xs)) and same_state(plan, ref)
    plan.close()
    ref.close()


# ---- against the float64 truth ------------------------------------------------------------------------------------------
def pair_figures(got, truth):
    """c per pair of outputs: max |got - truth| / (peak_a + peak_b), the peaks the truth's; got, truth [O][n]."""
    out = []
    for q in range(0, truth.shape[0], 2):
        rows = slice(q, min(q + 2, truth.shape[0]))
        out.append(np.abs(got[rows].astype(np.float64) - truth[rows]).max() / np.abs(truth[rows]).max(axis=1).sum())
    return np.array(out)


@functools.lru_cache(maxsize=None)
def truths(I, O, K, blocks):
    """(taps, x, y of the float32 restatement, y of the float64 truth): noise at unequal levels, decaying random taps"""
    taps, x = decaying_taps(O, I, K, 70 + K), noise(I, blocks * BLOCK, 50 + K)
    outs = []
    for wide in (False, True):
        twin = MconvTwin(I, O, K, wide)
        twin.set_taps(taps, ramp=False)
        outs.append(twin.process(x))
    return taps, x, outs[0], outs[1]


@pytest.mark.parametrize("I,O,K", [(5, 3, 1), (5, 3, 2), (5, 3, 3), (65, 3, 2)])
def test_the_outputs_are_within_4_c_twin_of_the_truth(gab, I, O, K):
    taps, x, narrow, wide = truths(I, O, K, 8)
    plan = started(gab, I, O, 1024, K, taps)
    y = run_stream(plan, x)
    c_dev, c_twin = pair_figures(y, wide), pair_figures(narrow, wide)
    print("mconv I=%d O=%d K=%d: c_dev %s c_twin %s ratio %s" % (I, O, K, c_dev, c_twin, c_dev / c_twin))
    assert (c_dev <= 4.0 * c_twin).all(), (c_dev, c_twin)
    plan.close()
