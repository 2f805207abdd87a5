"""The fdl scheme of the conv plan on the GPU: uniformly partitioned overlap-save with a frequency-domain delay line
(gab_conv_create_scheme, ConvPlan(..., scheme="fdl")) against the float64 whole-stream reference, bit identity of its
launch forms, its refusals, its real-time budget and the harness."""
import math

import numpy as np
import pytest

from test_conv_fdl_host import stream_reference

pytestmark = pytest.mark.gpu

TOL = 1e-5
CHUNK = 16          # buffers per batch launch: the delay line holds K + CHUNK - 1 spectra


@pytest.fixture(scope="module")
def gab():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gpuaudiobench_amd as g
    return g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reverb_ir(T, L, seed, tau=None):
    rng = np.random.default_rng(seed)
    tau = tau or max(L / 5.0, 1.0)
    return (rng.standard_normal((T, L)) * np.exp(-np.arange(L) / tau)).astype(np.float32).ravel()


def inputs(T, B, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(T * B).astype(np.float32) for _ in range(n)]


def wrap_len(B, L):
    """Buffers for the oldest partition to see real history and the delay line to wrap, plus 20."""
    K = math.ceil(L / B)
    return K + CHUNK - 1 + 20


def fdl_plan(gab, T, B, L, ir):
    p = gab.ConvPlan(T, B, L, scheme="fdl")
    p.set_ir(dev(ir))
    return p


def run_stream(plan, xs):
    return [host(plan.process(dev(x))) for x in xs]


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,T", [(512, 96000, 4), (512, 16385, 3), (256, 48000, 2), (2048, 300000, 2),
                                   (128, 5000, 5), (512, 512, 2), (512, 1, 1), (1024, 20000, 2)])
def test_streaming_matches_the_whole_stream_reference(gab, orc, B, L, T):
    ir = orc.conv_accel_ir(L, T) if (B, L) == (512, 16385) else reverb_ir(T, L, seed=L + T)
    xs = inputs(T, B, wrap_len(B, L), seed=B + T)
    plan = fdl_plan(gab, T, B, L, ir)
    assert plan.scheme == "fdl"
    ys = run_stream(plan, xs)
    plan.close()
    refs = stream_reference(xs, ir, T, B, L)
    peak = max(np.abs(r).max() for r in refs)
    errs = [np.abs(y - r).max() / peak for y, r in zip(ys, refs)]
    assert max(errs) <= TOL, (int(np.argmax(errs)), max(errs))
    first = orc.conv_accel(xs[0], ir, L, B, T)                # the golden: the first buffer from zero history
    assert np.abs(ys[0] - first).max() / np.abs(first).max() <= TOL


# 2 ------------------------------------------------------------------------------------------------------------------
def test_stateless_calls_match_the_golden_and_leave_the_stream_alone(gab, orc):
    T, B, L = 4, 512, 40000
    ir = reverb_ir(T, L, seed=2)
    xs = inputs(T, B, wrap_len(B, L), seed=3)
    a, b = fdl_plan(gab, T, B, L, ir), fdl_plan(gab, T, B, L, ir)
    ya = run_stream(a, xs)
    for i, x in enumerate(xs):
        yb = host(b.process(dev(x)))
        assert np.array_equal(bits(yb), bits(ya[i])), i
        if i % 7 == 0:
            z = xs[(i * 5 + 1) % len(xs)]
            ys = host(b.process(dev(z), mode=gab.CONV_STATELESS))
            g = orc.conv_accel(z, ir, L, B, T)
            assert np.abs(ys - g).max() / np.abs(g).max() <= TOL, i
    a.close()
    b.close()


# 3 ------------------------------------------------------------------------------------------------------------------
def batch_against_per_buffer(gab, T, B, L, n, seed):
    ir = reverb_ir(T, L, seed=seed)
    total = max(wrap_len(B, L), 2 * n + 10)
    xs = inputs(T, B, total, seed=seed + 1)
    a, b = fdl_plan(gab, T, B, L, ir), fdl_plan(gab, T, B, L, ir)
    ya = run_stream(a, xs)
    yb, i, turn = [], 0, 0
    while i < total:                                          # batches of n and runs of single buffers, mixed
        if turn % 2 == 0 and i + n <= total:
            out = host(b.process_batch(dev(np.concatenate(xs[i:i + n])), n))
            yb += list(out.reshape(n, T * B))
            i += n
        else:
            for _ in range(min(1 + turn % 3, total - i)):
                yb.append(host(b.process(dev(xs[i]))))
                i += 1
        turn += 1
    for k in range(total):
        assert np.array_equal(bits(yb[k]), bits(ya[k])), k
    a.close()
    b.close()


@pytest.mark.parametrize("n", [1, 7, 64])
def test_batch_is_bit_identical_to_per_buffer_calls(gab, n):
    # K = 40: two groups of the summation order; a (channel, bin) plane of 6 x 513 spreads them over threads
    batch_against_per_buffer(gab, 6, 512, 20000, n, seed=4)


@pytest.mark.parametrize("n", [7, 16])
def test_batch_is_bit_identical_in_the_walking_form(gab, n):
    # 512 x 513 >= 2^18 (channel, bin) entries: one thread walks both groups (K = 34) for all buffers of the batch
    batch_against_per_buffer(gab, 512, 512, 17000, n, seed=40)


# 4 ------------------------------------------------------------------------------------------------------------------
def test_channel_shard_gives_the_full_plans_columns(gab):
    # the full plan's (channel, bin) plane fills the device with one thread per bin; the shard's is small enough that
    # its partition groups go to separate threads: the same operations in the same order either way
    T, B, L, lo, hi = 600, 512, 20000, 64, 128
    ir = reverb_ir(T, L, seed=6)
    xs = inputs(T, B, 60, seed=7)
    full = fdl_plan(gab, T, B, L, ir)
    shard = fdl_plan(gab, hi - lo, B, L, ir.reshape(T, L)[lo:hi].ravel())
    for i, x in enumerate(xs):
        yf = host(full.process(dev(x))).reshape(B, T)[:, lo:hi]
        ys = host(shard.process(dev(x.reshape(T, B)[lo:hi].ravel()))).reshape(B, hi - lo)
        assert np.array_equal(bits(ys), bits(yf)), i
    full.close()
    shard.close()


# 5 ------------------------------------------------------------------------------------------------------------------
def test_reset_and_set_ir_mid_stream(gab):
    T, B, L = 5, 256, 12000
    ir1, ir2 = reverb_ir(T, L, seed=8), reverb_ir(T, L, seed=9)
    xs = inputs(T, B, 2 * wrap_len(B, L), seed=10)
    half = len(xs) // 2
    a = fdl_plan(gab, T, B, L, ir1)
    run_stream(a, xs[:17])
    a.reset()
    fresh = fdl_plan(gab, T, B, L, ir1)
    for x in xs[:half]:
        assert np.array_equal(bits(host(a.process(dev(x)))), bits(host(fresh.process(dev(x)))))
    # new taps from the next buffer on, for every partition at once
    b = fdl_plan(gab, T, B, L, ir2)
    run_stream(b, xs[:half])
    a.set_ir(dev(ir2))
    for i in range(half, len(xs)):
        assert np.array_equal(bits(host(a.process(dev(xs[i])))), bits(host(b.process(dev(xs[i]))))), i
    for p in (a, b, fresh):
        p.close()


# 6 ------------------------------------------------------------------------------------------------------------------
def test_pinned_host_buffers_give_the_same_bits(gab):
    import torch
    T, B, L = 8, 512, 30000
    ir = reverb_ir(T, L, seed=11)
    xs = inputs(T, B, wrap_len(B, L), seed=12)
    a, b = fdl_plan(gab, T, B, L, ir), fdl_plan(gab, T, B, L, ir)
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
    for i, x in enumerate(xs):
        ya = host(a.process(dev(x)))
        h_in.copy_(torch.from_numpy(x))
        b.process(h_in, out=h_out)
        torch.cuda.synchronize()
        assert np.array_equal(bits(h_out.numpy()), bits(ya)), i
    a.close()
    b.close()


# 7 ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_usable(gab):
    import torch
    T, B, L = 4, 512, 9000
    ir = reverb_ir(T, L, seed=13)
    xs = inputs(T, B, 30, seed=14)
    a, b = fdl_plan(gab, T, B, L, ir), fdl_plan(gab, T, B, L, ir)
    ya = run_stream(a, xs)
    yb = run_stream(b, xs[:10])
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
    calls = [lambda: b.round_trip(h_in, h_out), lambda: b.engine_start(4), lambda: b.newest_block(),
             lambda: b.set_scheme("classic"), lambda: b.set_scheme("split")]
    for call in calls:
        with pytest.raises(gab.GabError) as e:
            call()
        assert e.value.code == -1 and "fdl" in str(e.value)
    b.set_scheme("fdl")                                       # its own scheme: nothing changes
    assert b.scheme == "fdl"
    spectra, history = b.state_bytes()
    K, bins = math.ceil(L / B), B + 1
    assert spectra == 8 * K * T * bins
    assert history == 8 * (K + CHUNK - 1) * T * bins + 4 * T * B
    yb += run_stream(b, xs[10:])
    for i in range(len(xs)):
        assert np.array_equal(bits(yb[i]), bits(ya[i])), i
    a.close()
    b.close()


# 8 ------------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_uniform_partition_route(gab):
    T, B, L = 4, 512, 16384
    ir = reverb_ir(T, L, seed=15)
    xs = inputs(T, B, 40, seed=16)
    u = gab.ConvPlan(T, B, L)                                 # gab_conv_create's route for this shape
    u.set_ir(dev(ir))
    f = fdl_plan(gab, T, B, L, ir)
    yu, yf = run_stream(u, xs), run_stream(f, xs)
    peak = max(np.abs(y).max() for y in yu)
    assert max(np.abs(a - b).max() for a, b in zip(yf, yu)) / peak <= TOL
    u.close()
    f.close()


# 9 ------------------------------------------------------------------------------------------------------------------
def test_real_time_at_1024_channels_and_a_two_second_response(gab):
    import torch
    T, B, L = 1024, 512, 96000
    g = torch.Generator(device="cuda").manual_seed(17)
    ir = torch.randn(T, L, device="cuda", generator=g) * torch.exp(-torch.arange(L, device="cuda") / 19200.0)
    plan = gab.ConvPlan(T, B, L, scheme="fdl")
    plan.set_ir(ir.contiguous().view(-1))
    del ir
    x = torch.randn(8, T * B, device="cuda", generator=g)
    out = torch.empty(T * B, device="cuda")
    for i in range(10):
        plan.process(x[i % 8], out=out)
    times = []
    for i in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.process(x[i % 8], out=out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    plan.close()
    med = float(np.median(times))
    print("fdl T=1024 B=512 L=96000: median %.3f ms per buffer (budget 10.67 ms)" % med)
    assert med < 2.0, times


# 10 -----------------------------------------------------------------------------------------------------------------
def test_harness_runs_the_fdl_scheme(gab):
    b = gab.Benchmark("Conv1D_accel", n_tracks=64, buffer_size=512, ir_length=20000,
                      conv_mode=gab.CONV_STREAMING, conv_scheme=2)
    b.setup()
    r = b.run(iterations=20, warmup=3)
    v, text = b.validate()
    assert v.status == 0 and v.max_error <= TOL, text
    assert r.gpu_median_ms > 0
    b.close()
    rt = gab.Benchmark("Conv1D_accel", n_tracks=64, buffer_size=512, ir_length=20000, conv_mode=2, conv_scheme=2)
    with pytest.raises(gab.GabError) as e:
        rt.setup()
    assert "fdl" in str(e.value)
    rt.close()
