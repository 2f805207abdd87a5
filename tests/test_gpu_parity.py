"""GPU parity: every HIP kernel, called through the C ABI, against the CPU oracle.

Bar (BASELINE.json north_star): bit-exact for gain / rndmem / index work, and
<= 1e-5 relative for float DSP.  "Relative" is peak-normalised,
max|gpu - ref| / max|ref| (element-wise relative error is
meaningless at zero crossings).  Kernels that keep the golden's operation order
(iir, conv1d, dwg, fdtd3d) are additionally required to be bit-identical.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5


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


def peak_err(got, ref):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------
def test_gain_bit_exact(gab, orc):
    x = orc.noise(128 * 512)
    y = host(gab.gain(dev(x), 2.0))
    assert np.array_equal(bits(y), bits(orc.gain(x, 2.0)))
    assert orc.fnv_survey(y) == "74d41e0b3a202944"          # SURVEY §8c pin, C1


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1027, 65537])
def test_gain_ragged_and_unaligned(gab, orc, n):
    x = orc.noise(n + 1)
    y = host(gab.gain(dev(x)[:n].contiguous(), 0.37))
    assert np.array_equal(bits(y), bits(orc.gain(x[:n], 0.37)))
    # unaligned base pointer: a view that starts 4 bytes in
    import torch
    xd = dev(x)
    out = torch.empty(n + 1, device="cuda")
    gab.gain(xd[1:], 0.37, out=out[1:])
    assert np.array_equal(bits(host(out[1:])), bits(orc.gain(x[1:], 0.37)))


def test_gain_empty(gab):
    import torch
    y = gab.gain(torch.empty(0, device="cuda"), 2.0)
    assert y.numel() == 0


def test_noop(gab, orc):
    x = orc.noise(128 * 512 + 3)
    assert np.array_equal(bits(host(gab.noop(dev(x)))), bits(x))


@pytest.mark.parametrize("T,B", [(128, 512), (3, 511), (130, 64), (1, 7)])
def test_gainstats(gab, orc, T, B):
    x = orc.noise(T * B)
    y, st = gab.gainstats(dev(x), T, B)
    ry, rs = orc.gainstats(x, T, B)
    assert np.array_equal(bits(host(y)), bits(ry))                 # scaled output exact
    st = host(st).reshape(T, 2)
    rs = rs.reshape(T, 2)
    assert np.array_equal(bits(st[:, 1]), bits(rs[:, 1]))          # max exact
    # mean: wave butterfly order != sequential order; sums are O(10), means O(1e-2)
    assert np.abs(st[:, 0] - rs[:, 0]).max() <= TOL * max(np.abs(rs[:, 0]).max(), 1e-3)


@pytest.mark.parametrize("rin,rout", [(0.2, 0.8), (0.99, 0.01), (0.01, 0.99)])
def test_datatransfer(gab, orc, rin, rout):
    n_in, n_out = orc.datatransfer_size(rin), orc.datatransfer_size(rout)
    x = orc.Rand(1).unit(n_in)
    y = host(gab.datatransfer(dev(x), n_out))
    ref = orc.datatransfer(x, n_out)
    m = min(n_in, n_out)
    assert np.array_equal(bits(y[:m]), bits(ref[:m]))              # the copied part is exact
    assert peak_err(y, ref) <= TOL


@pytest.mark.parametrize("n_in,n_out", [(26214, 2595225), (524288, 2097152), (1310720, 1310720), (2097152, 524288),
                                        (2595225, 26214), (1, 1), (3, 7), (7, 3), (1025, 1023), (0, 5000), (4097, 0),
                                        (1024, 1024), (5000, 4096)])
def test_datatransfer_round_trip_is_the_device_kernel_bit_for_bit(gab, orc, n_in, n_out):
    """Upload and download at once (gab_datatransfer_round_trip) against the device-buffer kernel on the same input:
    identical bits, ragged sizes included; the copied part equals the input exactly.  The plan is reused."""
    import torch
    plan = gab.LinkPlan(max(n_in, 1))
    for rep in range(3):
        x = orc.Rand(1 + rep).unit(n_in)
        h_in = torch.from_numpy(x).pin_memory()
        h_out = torch.full((n_out,), -7.0).pin_memory()
        plan.round_trip(h_in, h_out)
        ref = host(gab.datatransfer(dev(x), n_out)) if n_out else np.zeros(0, np.float32)
        assert np.array_equal(bits(h_out.numpy()), bits(ref)), "call %d" % rep
        m = min(n_in, n_out)
        assert np.array_equal(bits(h_out.numpy()[:m]), bits(x[:m]))
        assert peak_err(h_out.numpy(), orc.datatransfer(x, n_out)) <= TOL if n_out else True
    plan.close()


def test_datatransfer_round_trip_input_that_holds_the_sentinel_and_smaller_calls(gab, orc):
    """Input words that really are the staging sentinel are released by the upload's event (slower, never wrong);
    a later, shorter call on the same plan does not see what an earlier, longer one left behind."""
    import torch
    n = 300000
    plan = gab.LinkPlan(n)
    x = orc.Rand(5).unit(n)
    xb = x.view(np.uint32).copy()
    xb[::7] = 0xffa5c3e1
    xb[-1] = 0xffa5c3e1
    h_in = torch.from_numpy(xb.view(np.float32).copy()).pin_memory()
    h_out = torch.zeros(n + 1000).pin_memory()
    for _ in range(2):
        plan.round_trip(h_in, h_out)
        assert np.array_equal(bits(h_out.numpy()[:n]), xb)
    for m_in, m_out in ((1000, 200000), (123457, 123457), (n, 10), (n, n), (n - 5, 77), (n, n + 9), (50, 0), (n, 3000)):
        y = orc.Rand(m_in).unit(m_in)
        h_o = torch.zeros(m_out).pin_memory()
        plan.round_trip(torch.from_numpy(y).pin_memory(), h_o)
        assert np.array_equal(bits(h_o.numpy()), bits(host(gab.datatransfer(dev(y), m_out))))
    with pytest.raises(gab.GabError):
        plan.round_trip(torch.zeros(n + 1).pin_memory(), h_out)          # longer than the plan
    with pytest.raises(TypeError):
        plan.round_trip(h_in, torch.zeros(16))                           # pageable output
    plan.close()


@pytest.mark.parametrize("T,B", [(128, 512), (5, 100), (200, 513)])
def test_iir_sequential_bit_exact_with_carried_state(gab, orc, T, B):
    c = orc.iir_coeffs(0.25)
    x = orc.noise(T * B)
    st_ref = np.zeros(2 * T, np.float32)
    st = dev(np.zeros(2 * T, np.float32))
    for it in range(3):                                   # state carries across buffers
        xi = np.roll(x, it * 17)
        y = host(gab.iir(dev(xi), c, st, T, B, sequential=True))
        ry = orc.iir(xi, c, st_ref, T, B)
        assert np.array_equal(bits(y), bits(ry)), "buffer %d" % it
        assert np.array_equal(bits(host(st)), bits(st_ref))
    if (T, B) == (128, 512):
        st0 = np.zeros(2 * T, np.float32)
        assert orc.fnv_survey(orc.iir(x, c, st0, T, B)) == "fad0d0724cb98566"


@pytest.mark.parametrize("T,B", [(128, 512), (3, 64), (1000, 128), (7, 1024), (130, 256),
                                 (16384, 512), (16387, 1024)])     # many tracks: the scan runs in 256-sample segments
def test_iir_wave_scan_with_carried_state(gab, orc, T, B):
    """The wave-scan kernel re-associates the recurrence: gated at 1e-5 of peak
    (measured ~1e-7), outputs and carried state, over several buffers."""
    c = orc.iir_coeffs(0.25)
    x = orc.noise(T * B)
    st_ref = np.zeros(2 * T, np.float32)
    st = dev(np.zeros(2 * T, np.float32))
    for it in range(4):
        xi = np.roll(x, it * 29)
        y = host(gab.iir(dev(xi), c, st, T, B))
        ry = orc.iir(xi, c, st_ref, T, B)
        assert peak_err(y, ry) <= TOL, (it, peak_err(y, ry))
        assert peak_err(host(st), st_ref) <= TOL
    # a different filter (narrow band-pass-like poles closer to the unit circle)
    c2 = np.array([0.2, 0.1, -0.05, -1.2, 0.72], np.float32)
    st_ref[:] = 0
    st = dev(np.zeros(2 * T, np.float32))
    for it in range(2):
        y = host(gab.iir(dev(x), c2, st, T, B))
        ry = orc.iir(x, c2, st_ref, T, B)
        assert peak_err(y, ry) <= TOL


@pytest.mark.parametrize("L,T,B", [(256, 256, 512), (1024, 16, 512), (100, 7, 300), (1500, 3, 64)])
def test_conv1d_bit_exact(gab, orc, L, T, B):
    ir = orc.conv1d_ir(L, T)
    x = orc.noise(T * B)
    y = host(gab.conv1d(dev(x), dev(ir), L, T, B))
    ref = orc.conv1d(x, ir, L, B, T)
    assert peak_err(y, ref) <= TOL
    assert np.array_equal(bits(y), bits(ref))
    if (L, T, B) == (256, 256, 512):
        assert orc.fnv_survey(y) == "f66260025b0fa20c"           # SURVEY §8c pin, C2


@pytest.mark.parametrize("L", [1, 15, 31, 32, 33, 63, 64, 65, 95, 96, 127, 1041, 2080])
def test_conv1d_group_remainders_bit_exact(gab, orc, L):
    """Every remainder of the 32-tap groups the chain is cut into, below one group, across the 1024-tap chunks, with
    a ragged last tile (B = 300) and tiles at the start of the stream (taps that reach before sample 0)."""
    T, B = 5, 300
    ir = orc.conv1d_ir(L, T)
    x = orc.noise(T * B, seed=L)
    y = host(gab.conv1d(dev(x), dev(ir), L, T, B))
    assert np.array_equal(bits(y), bits(orc.conv1d(x, ir, L, B, T)))


def test_conv1d_start_of_stream_skips_taps_also_when_they_are_not_finite(gab, orc):
    """The golden SKIPS a tap that reaches before sample 0 (cuda/bench_conv1d.cu:188-208).  With finite taps the kernel
    lets the window's zeros do that; a response that holds an infinity or a NaN must take the chain with the select:
    inf x 0 would be NaN where the golden has a number.  Also: signed zeros in input and taps."""
    T, B, L = 6, 512, 300
    ir = orc.conv1d_ir(L, T)
    ir[0 * L + 7] = np.inf
    ir[1 * L + 0] = np.nan
    ir[2 * L + 299] = -np.inf
    ir[3 * L + 11] = -0.0
    x = orc.noise(T * B, seed=9)
    x[::13] = -0.0
    x[5::17] = 0.0
    y = host(gab.conv1d(dev(x), dev(ir), L, T, B))
    ref = orc.conv1d(x, ir, L, B, T)
    nan_y, nan_r = np.isnan(y), np.isnan(ref)
    assert np.array_equal(nan_y, nan_r)
    assert np.array_equal(bits(y)[~nan_y], bits(ref)[~nan_r])
    assert np.isfinite(ref[:7]).all()                     # the golden has numbers there: the infinite tap is skipped


def where_bits_differ(a, b, T):
    """'' when the two sample-major [B][T] outputs are the same bits; else WHERE they differ (for an assertion message: a
    mismatch that cannot be made to happen again should at least say which rows and channels it was)."""
    d = bits(a) != bits(b)
    if not d.any():
        return ""
    idx = np.flatnonzero(d)
    smp, ch = idx // T, idx % T
    return ("%d words differ: samples %d..%d (%d distinct), channels %d..%d (%d distinct); NaN in a: %d, in b: %d; first at %d: %r vs %r"
            % (idx.size, smp.min(), smp.max(), np.unique(smp).size, ch.min(), ch.max(), np.unique(ch).size,
               int(np.isnan(np.asarray(a)).sum()), int(np.isnan(np.asarray(b)).sum()), idx[0], np.asarray(a).ravel()[idx[0]], np.asarray(b).ravel()[idx[0]]))


# ---------------------------------------------------------------------------
# conv1d_accel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L,T", [(4096, 64), (512, 128), (256, 6), (4096, 5), (700, 2), (1, 2)])
def test_conv_accel_reference_semantics(gab, orc, L, T):
    B = 512
    ir = orc.conv_accel_ir(L, T) if L > 1 else np.ones(T, np.float32)
    x = orc.noise(T * B)
    ref = orc.conv_accel(x, ir, L, B, T)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    y0 = host(plan.process(dev(x), mode=gab.CONV_STATELESS))
    assert peak_err(y0, ref) <= TOL
    # a freshly reset streaming plan gives the same first buffer: to the bit with the classic cut
    # of the taps, to rounding with the split one (where the shape has it)
    for scheme in ("classic", "split"):
        plan.reset()
        try:
            plan.set_scheme(scheme)
        except gab.GabError:
            assert scheme == "split" and not (L > 1024 and T % 4 == 0)
            continue
        assert plan.scheme == scheme
        y1 = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        assert peak_err(y1, ref) <= TOL
        if scheme == "classic":
            assert np.array_equal(bits(y0), bits(y1))
    plan.close()


def test_conv_accel_c3_full_size(gab, orc):
    T, B, L = 1024, 512, 4096
    ir = orc.conv_accel_ir(L, T)
    x = orc.noise(T * B)
    ref = orc.conv_accel(x, ir, L, B, T)
    assert orc.fnv_survey(ref) == "6931c469f45f4d0e"             # SURVEY §8c pin, C3
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
    assert peak_err(y, ref) <= TOL
    plan.close()


@pytest.mark.parametrize("L,T,nbuf", [(4096, 16, 12), (512, 9, 4), (2000, 4, 10)])
def test_conv_accel_streaming_vs_direct_form(gab, orc, L, T, nbuf):
    """Beyond the first buffer the reference pins nothing; the oracle is its golden
    extended with carried history (float64 accumulation as truth).

    Normalisation: the first buffer (reference semantics) is gated on its own
    peak.  Later buffers are gated on the STREAM's peak: for the 7 buffers after
    a reset the 4096-point window is still partly zeros, outputs are ~1e-6 (only
    the tiny leading taps are reached) while FFT round-off scales with the large
    centre taps, so a per-buffer ratio there measures the onset, not the kernel
    (measured: abs error <= 3e-10 against a 1e-3 steady-state signal).  Once the
    window is full (buffer 8 on) the per-buffer ratio is gated as well."""
    B = 512
    ir = orc.conv_accel_ir(L, T)
    hist = np.zeros(T * L, np.float32)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    max_abs, stream_peak = 0.0, 0.0
    for n in range(nbuf):
        x = orc.noise(T * B, seed=100 + n)
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        if n == 0 or n >= 8:
            assert peak_err(y, ref) <= TOL, (n, peak_err(y, ref))
        max_abs = max(max_abs, np.abs(y - ref).max())
        stream_peak = max(stream_peak, np.abs(ref).max())
    assert max_abs / stream_peak <= TOL, max_abs / stream_peak
    # reset really forgets
    plan.reset()
    x = orc.noise(T * B)
    y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
    assert peak_err(y, orc.conv_accel(x, ir, L, B, T)) <= TOL
    plan.close()


def test_conv_accel_linearity_and_shard_equality(gab, orc):
    """Size-independent properties at the full C3 shape: (a) conv(a*x1 + x2) =
    a*conv(x1) + conv(x2); (b) processing channels [256,512) alone, with the IR
    slice of the GLOBAL bank, reproduces those channels of the full run bit for
    bit (what multi-GPU sharding relies on)."""
    T, B, L = 1024, 512, 4096
    ir = orc.conv_accel_ir(L, T)
    full = gab.ConvPlan(T, B, L)
    full.set_ir(dev(ir))
    outs = []
    xs = [orc.noise(T * B, seed=s) for s in (1, 2)]
    for xv in (xs[0], xs[1], (0.5 * xs[0] + xs[1]).astype(np.float32)):
        full.reset()
        for _ in range(9):                                    # history window full (steady state)
            y = host(full.process(dev(xv), mode=gab.CONV_STREAMING))
        outs.append(y.astype(np.float64))
    lin = np.abs(outs[2] - (0.5 * outs[0] + outs[1])).max() / np.abs(outs[2]).max()
    assert lin <= TOL
    lo, hi = 256, 512
    ir_slice = orc.conv_accel_ir(L, hi - lo, track_offset=lo, total_tracks=T)
    assert np.array_equal(ir_slice, ir.reshape(T, L)[lo:hi].ravel())
    shard = gab.ConvPlan(hi - lo, B, L)
    shard.set_ir(dev(ir_slice))
    xs0 = xs[0].reshape(T, B)[lo:hi].ravel()
    for _ in range(9):
        ys = host(shard.process(dev(xs0), mode=gab.CONV_STREAMING))
    assert np.array_equal(bits(ys.reshape(B, hi - lo)), bits(outs[0].astype(np.float32).reshape(B, T)[:, lo:hi]))
    full.close()
    shard.close()


@pytest.mark.parametrize("B,L,T,nbuf", [
    (256, 512, 8, 6), (128, 1000, 3, 12), (1024, 6000, 2, 9),      # the reference takes any (ir_length, buffer_size)
    (512, 8192, 4, 20), (512, 16384, 2, 36),                        # longer than one 4096-point window: 3 and 5 partitions
    (256, 4096, 64, 20), (64, 4096, 5, 70), (32, 700, 3, 40), (2048, 3000, 2, 4),
    (1024, 16384, 1, 20), (128, 16384, 2, 140),
])
def test_conv_accel_uniform_partitions(gab, orc, B, L, T, nbuf):
    """Every other power-of-two buffer size and impulse responses up to 16384 taps run fused as well
    (conv_uniform_kernel: partitions of 4096 - B taps, one 4096-point transform each, one inverse):
    reference semantics on a stateless call, and a stream long enough for the oldest partition's
    window to fill, against the float64 direct form (cuda/bench_conv1d_accel.cu:234-252 extended
    with carried history); reset forgets."""
    ir = orc.conv_accel_ir(L, T)
    hist = np.zeros(T * L, np.float32)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    x = orc.noise(T * B)
    assert peak_err(host(plan.process(dev(x), mode=gab.CONV_STATELESS)),
                    orc.conv_accel(x, ir, L, B, T)) <= TOL
    max_abs, stream_peak = 0.0, 0.0
    full = (L + B - 1) // B                                   # buffers until every tap sees real history
    for n in range(nbuf):
        x = orc.noise(T * B, seed=7 + n)
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        if n == 0 or n >= full:
            assert peak_err(y, ref) <= TOL, (n, peak_err(y, ref))
        max_abs = max(max_abs, np.abs(y - ref).max())
        stream_peak = max(stream_peak, np.abs(ref).max())
    assert nbuf > full or L > 8 * B
    assert max_abs / stream_peak <= TOL
    plan.reset()
    x = orc.noise(T * B, seed=99)
    y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
    assert peak_err(y, orc.conv_accel(x, ir, L, B, T)) <= TOL
    plan.close()


@pytest.mark.parametrize("B,L,T", [(300, 700, 3), (48, 100, 2), (4096, 512, 1)])
def test_conv_accel_direct_form_last_resort(gab, orc, B, L, T):
    """Buffer sizes that are not a power of two (or beyond 2048) keep the direct-form kernel."""
    ir = orc.conv_accel_ir(L, T)
    hist = np.zeros(T * L, np.float32)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    x = orc.noise(T * B)
    assert peak_err(host(plan.process(dev(x), mode=gab.CONV_STATELESS)),
                    orc.conv_accel(x, ir, L, B, T)) <= TOL
    max_abs, stream_peak = 0.0, 0.0
    for n in range(4):
        x = orc.noise(T * B, seed=7 + n)
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        max_abs = max(max_abs, np.abs(y - ref).max())
        stream_peak = max(stream_peak, np.abs(ref).max())
    assert max_abs / stream_peak <= TOL
    plan.close()


def test_conv_accel_zero_copy_pinned_host_buffers(gab, orc):
    """d_in / d_out may be pinned host memory: the kernel then moves the buffer over PCIe itself.
    Same bits as with device buffers and copy commands."""
    import torch
    T, B, L = 64, 512, 4096
    ir = dev(orc.conv_accel_ir(L, T))
    xs = [orc.noise(T * B, seed=30 + i) for i in range(4)]
    h_out = torch.empty(T * B).pin_memory()
    for scheme in ("split", "classic"):               # a host-io launch runs the plan's own cut
        a, b = gab.ConvPlan(T, B, L, scheme=scheme), gab.ConvPlan(T, B, L, scheme=scheme)
        a.set_ir(ir)
        b.set_ir(ir)
        for x in xs:
            ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
            b.process(torch.from_numpy(x).pin_memory(), out=h_out, mode=gab.CONV_STREAMING)
            torch.cuda.synchronize()
            assert b.scheme == scheme
            assert np.array_equal(bits(ya), bits(h_out.numpy()))
        with pytest.raises(TypeError):
            a.process(torch.from_numpy(xs[0]))        # pageable host memory is not device-accessible
        a.close()
        b.close()


@pytest.mark.parametrize("T,L,n", [(64, 4096, 12), (1024, 4096, 12), (8, 1500, 10),
                                   (2052, 3000, 40),     # 4.2 MB of input: ONE word straddles the runtime's 4 MiB - 1 byte engine-packet limit (r05_incident_torn_word.txt)
                                   (8192, 4096, 4)])     # three such words
def test_conv_accel_round_trip_overlapped_link_same_bits_as_device_buffers(gab, orc, T, L, n):
    """gab_conv_round_trip on the classic cut (engine upload consumed as it lands, far partition before the
    input, outputs drained per channel group): bit for bit what device-buffer launches of the same cut give,
    over more buffers than the history holds, alone and mixed with device-buffer launches on the SAME plan;
    the steady state also against the oracle's float64 direct form."""
    import torch
    B = 512
    ir_h = orc.conv_accel_ir(L, T)
    ir = dev(ir_h)
    a, b = gab.ConvPlan(T, B, L, scheme="classic"), gab.ConvPlan(T, B, L, scheme="classic")
    a.set_ir(ir)
    b.set_ir(ir)
    h_in = torch.empty(T * B).pin_memory()
    h_out = torch.empty(T * B).pin_memory()
    hist = np.zeros(T * L, np.float32)
    worst = peak = 0.0
    prev = {"out": None, "in": None}

    def compared_round_trip(x, src, label):
        """One gab_conv_round_trip against the device-buffer launch of the same input, set up so that a single
        mismatch says which hand-off failed (tests/rt_diag.py): NaN-filled output, the consumed block read back."""
        ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
        h_out.fill_(float("nan"))
        yb = b.round_trip(src, h_out).numpy().copy()
        consumed = host(b.newest_block())
        report = rt_diag.classify(ya, yb, T, B, prev_out=prev["out"], h_in=x, consumed=consumed, prev_in=prev["in"], label=label)
        assert not report, report
        prev["out"], prev["in"] = yb, x
        return yb

    import rt_diag
    for i in range(n):
        x = orc.noise(T * B, seed=90 + i)
        if i % 5 == 3:                                   # a device-buffer launch in the middle of the stream
            ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
            yb = host(b.process(dev(x), mode=gab.CONV_STREAMING))
            assert not where_bits_differ(ya, yb, T), "buffer %d: %s" % (i, where_bits_differ(ya, yb, T))
            prev["out"], prev["in"] = yb, x
        else:
            h_in.copy_(torch.from_numpy(x))
            yb = compared_round_trip(x, h_in, "buffer %d" % i)     # complete when the call returns: no synchronize here
        if T <= 64:
            ref = orc.conv_accel_stream(x, ir_h, hist, L, B, T, f64=True)
            worst, peak = max(worst, float(np.abs(yb - ref).max())), max(peak, float(np.abs(ref).max()))
    if T <= 64:
        assert worst / peak <= 1e-5
    # a pageable input: uploaded completely before the launch
    x = orc.noise(T * B, seed=8)
    compared_round_trip(x, torch.from_numpy(x.copy()), "pageable input")
    # the staging buffer is re-armed after every buffer: the same input twice in a row is two buffers, not one
    x = orc.noise(T * B, seed=7)
    h_in.copy_(torch.from_numpy(x))
    for k in range(2):
        compared_round_trip(x, h_in, "same input, call %d" % k)
    a.close()
    b.close()


def test_keep_warm_launch_comes_and_goes_and_changes_no_bits(gab, orc):
    """gab_keep_warm: a kick starts the resident launch, later kicks push its end out, it ends by itself idle_seconds after
    the last one and a kick brings it back; a plan whose round trips kick one (gab_conv_round_trip_keep_warm) gives the
    same bits as one that does not, also while a keep-warm of the widest shape sits on the device; destroying a plan or
    a keep-warm with the launch still there returns at once (the stop word, not the idle limit)."""
    import time, torch
    w = gab.KeepWarm(workgroups=256, idle_seconds=0.05)
    assert not w.running()
    w.kick()
    assert w.running()
    for _ in range(10):                                  # 0.1 s of kicks: twice the idle limit
        time.sleep(0.01)
        w.kick()
    assert w.running()
    time.sleep(0.3)
    assert not w.running()
    w.kick()
    assert w.running()
    T, B, L = 64, 512, 4096
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="classic"), gab.ConvPlan(T, B, L, scheme="classic")
    a.set_ir(ir)
    b.set_ir(ir)
    b.round_trip_keep_warm(True)
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
    for i in range(12):
        x = orc.noise(T * B, seed=300 + i)
        h_in.copy_(torch.from_numpy(x))
        ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
        yb = b.round_trip(h_in, h_out).numpy()
        assert not where_bits_differ(ya, yb, T), "buffer %d: %s" % (i, where_bits_differ(ya, yb, T))
        w.kick()
    b.close()                                            # its launch is still there: the stop word ends it
    w.close()
    w = gab.KeepWarm(workgroups=8, idle_seconds=2.0)
    assert w.placement() == []                           # nothing has started
    w.kick()
    t0 = time.perf_counter()
    while len(w.placement()) < 8 and time.perf_counter() - t0 < 2.0:
        time.sleep(0.001)
    where = w.placement()                                # every wave says where it landed (HW_ID / XCC_ID)
    assert len(where) == 8 and all(0 <= p["xcc"] < 8 and 0 <= p["cu"] < 16 for p in where), where
    assert len({(p["xcc"], p["se"], p["sa"], p["cu"], p["simd"], p["slot"]) for p in where}) == 8, where   # eight different wave slots
    print("keep-warm placement:", gab.ops.placement_summary(where))
    t0 = time.perf_counter()
    w.close()                                            # the stop word, not the idle limit
    assert time.perf_counter() - t0 < 0.5
    a.close()
    with pytest.raises(gab.GabError):
        gab.KeepWarm(workgroups=0)
    with pytest.raises(gab.GabError):
        gab.KeepWarm(workgroups=8, idle_seconds=0.0)


def test_conv_accel_round_trip_reports_a_word_consumed_with_the_wrong_value(gab, orc):
    """The overlapped round trip takes input words while the upload is still running; that rests on engine writes landing
    whole and once (an observation: profiles/r05_incident_torn_word.txt was a violation nobody reported).  Since round 6 a
    check launch behind every call, ordered behind the upload's completion event, compares the consumed words with what the
    COMPLETED upload left: a diagnostic build that shows the kernel one wrong bit early (GAB_RT_TEAR; three word positions)
    must get GAB_ERR_RUNTIME — from gab_conv_round_trip_check, from a following call, and with set_check(2) at that call — and be
    right again after a reset (tools/round_trip_tear_check.py, a child process: the variable is read by the library)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "gpuaudiobench_amd", "libgab_hip_ablate.so")
    if not os.path.exists(lib):
        pytest.skip("no diagnostic build")
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "round_trip_tear_check.py")], cwd=root,
                       env=dict(os.environ, GAB_LIB_PATH=lib), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert all(k in r.stdout for k in ("by round_trip_check", "at that call", "by a following call", "bit for bit: ok")), r.stdout


def test_conv_accel_round_trip_input_that_holds_the_sentinel(gab, orc):
    """A buffer that really contains the staging sentinel (a NaN no audio carries) is released by the upload's
    completion instead of by the words changing: slower, same bits as the device-buffer launch (NaNs and all)."""
    import torch
    T, B, L = 16, 512, 4096
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="classic"), gab.ConvPlan(T, B, L, scheme="classic")
    a.set_ir(ir)
    b.set_ir(ir)
    x = orc.noise(T * B, seed=3)
    xs = x.view(np.uint32).copy()
    xs[B - 1] = 0xffa5c3e1                               # one thread's word
    xs[2 * B - 1] = 0xffa5c3e1                           # the word the coarse poll watches
    xs[5 * B + 17] = 0xffa5c3e1
    # "landed" is judged by a word's top byte (a word cut by an engine-packet boundary shows the sentinel's high bytes over the
    # input's low ones for a moment): any input word whose own top byte is 0xff takes the same slow path — minus infinity, a
    # huge negative number, another negative NaN
    xs[8 * B + 3] = 0xff800000                           # -inf: channel pair 4
    xs[11 * B + 500] = 0xff000001                        # about -1.7e38 (finite): channel pair 5
    x = xs.view(np.float32)
    h_in = torch.from_numpy(x.copy()).pin_memory()
    h_out = torch.empty(T * B).pin_memory()
    for i in range(3):
        ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
        yb = b.round_trip(h_in, h_out).numpy()
        assert np.array_equal(bits(host(b.newest_block())), xs), "buffer %d: the consumed block" % i
        # the channel pairs that saw a NaN or an infinity are not finite in both (which NaN depends on operand order, which
        # two compilations of the same arithmetic need not share); every other channel is the same bits
        bad = ~np.isfinite(ya)
        assert np.array_equal(bad, ~np.isfinite(yb)), "buffer %d" % i
        assert bad.reshape(B, T)[:, [0, 1, 4, 5, 8, 9]].all() and not bad.reshape(B, T)[:, [2, 3, 6, 7, 12, 15]].any()
        assert np.array_equal(bits(ya)[~bad], bits(yb)[~bad]), "buffer %d" % i
    a.close()
    b.close()


def test_conv_accel_round_trip_other_plans_and_arguments(gab, orc):
    """Plans the overlapped form does not cover (split cut, other buffer sizes) move the buffers by the kernel
    itself and still return a complete output; the output must be pinned."""
    import torch
    for T, B, L, scheme in ((64, 512, 4096, "split"), (6, 256, 700, None), (6, 512, 300, None)):
        ir = dev(orc.conv_accel_ir(L, T))
        a, b = gab.ConvPlan(T, B, L, scheme=scheme), gab.ConvPlan(T, B, L, scheme=scheme)
        a.set_ir(ir)
        b.set_ir(ir)
        h_out = torch.empty(T * B).pin_memory()
        for i in range(3):
            x = orc.noise(T * B, seed=60 + i)
            ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
            yb = b.round_trip(torch.from_numpy(x).pin_memory(), h_out).numpy()
            assert np.array_equal(bits(ya), bits(yb))
        with pytest.raises(TypeError):
            b.round_trip(torch.from_numpy(x).pin_memory(), torch.empty(T * B))       # pageable output
        with pytest.raises(gab.GabError):
            b.round_trip(torch.from_numpy(x.copy()), h_out)       # these plans' kernels read the input themselves: pageable is refused, not dereferenced
        a.close()
        b.close()


def test_conv_accel_engine_fed_through_the_doorbell_same_bits(gab, orc):
    """gab_conv_engine_*: one resident launch that takes buffers as they are published.  An eight-slot ring refilled by
    copies WHILE the launch runs (so the launch must see fresh data in a slot it has read before), one buffer per ring
    of the doorbell, slots reused only after their buffer came back; every output bit for bit what one
    gab_conv_process launch per buffer gives, the history carried on into ordinary launches after the stop."""
    import torch
    T, B, L, R, N = 64, 512, 4096, 8, 30
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    xs = [orc.noise(T * B, seed=200 + i) for i in range(N + 2)]     # (a buffer comes back once five more are published: the ring holds eight)
    want = [host(a.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
    # two ordinary launches first: the engine starts from a history that is not empty
    for k in range(2):
        assert np.array_equal(bits(host(b.process(dev(xs[k]), mode=gab.CONV_STREAMING))), bits(want[k]))
    side = torch.cuda.Stream()                       # the engine owns its stream until stop
    in_ring, out_ring = b.engine_start(R, stream=side)
    cur = torch.cuda.current_stream()
    got = {}

    def collect():
        done = b.engine_completed()
        for k in range(len(got), done):
            got[k] = out_ring[k % R].cpu().numpy().copy()          # a copy on the default stream: the slot is complete
        return done

    import time
    for k in range(N):
        t0 = time.time()
        while k - collect() >= R:                    # slot k % R still holds an output nobody has taken / an input in use
            assert time.time() - t0 < 20, "the engine stopped returning buffers (completed %d of %d published)" % (len(got), k)
        in_ring[k % R].copy_(torch.from_numpy(xs[2 + k]).pin_memory(), non_blocking=True)   # a copy ENGINE's work
        cur.synchronize()                            # the slot is written before the doorbell rings
        b.engine_publish(1)
    for call in (lambda: b.process(dev(xs[0])), b.reset, lambda: b.process_batch(dev(np.concatenate(xs[:2])), 2)):
        with pytest.raises(gab.GabError):            # the running engine owns the plan's history
            call()
    b.engine_stop()                                  # everything published is finished when this returns
    assert collect() == N
    for k in range(N):
        assert np.array_equal(bits(got[k]), bits(want[2 + k])), "buffer %d" % k
    with pytest.raises(gab.GabError):
        b.engine_publish(1)                          # no running engine
    a.close()
    b.close()


@pytest.mark.parametrize("T", [64, 1024])
def test_conv_accel_engine_one_buffer_in_flight(gab, orc, T):
    """The real-time form of the engine (cuda/bench_conv1d_accel.cu:258-304 takes ONE buffer per iteration): the host
    writes buffer k into its slot, rings the doorbell WITH the flush rung, waits for `completed` = k + 1 and only then
    produces buffer k + 1 — nothing else is ever pending.  Every output bit for bit what one gab_conv_process launch per
    buffer gives: 50 buffers back to back, 12 paced at 512/48000 s, then a pipelined stretch (six published at once) and
    single buffers again on the SAME launch — bursts of any length walk one history — and ordinary launches after the stop."""
    import time
    import torch
    B, L, R = 512, 4096, 8
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    N = 50 + 12 + 6 + 5
    xs = [orc.noise(T * B, seed=400 + i) for i in range(N + 1)]
    want = [host(a.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
    side = torch.cuda.Stream()
    in_ring, out_ring = b.engine_start(R, stream=side)
    cur = torch.cuda.current_stream()
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()

    def put(k):                                      # copy ENGINES move the slots: at 1024 channels the launch holds every compute unit
        h_in.copy_(torch.from_numpy(xs[k]))
        in_ring[k % R].copy_(h_in, non_blocking=True)
        cur.synchronize()

    def take(k):
        h_out.copy_(out_ring[k % R], non_blocking=True)
        cur.synchronize()
        assert np.array_equal(bits(h_out.numpy()), bits(want[k])), "buffer %d" % k

    k = 0
    for _ in range(50):                              # back to back, one in flight
        put(k)
        b.engine_submit(1, flush=True)
        b.engine_wait(k + 1, timeout=8.0)
        assert b.engine_completed() == k + 1
        take(k)
        k += 1
    daw = gab.harness.DawSim(buffer_seconds=float(B) / 48000, mode="spin")
    for _ in range(12):                              # one buffer per 10.667 ms slot: the engine idles in between
        daw.wait()
        put(k)
        t0 = time.perf_counter()
        b.engine_submit(1, flush=True)
        b.engine_wait(k + 1, timeout=8.0)
        assert time.perf_counter() - t0 < 0.010667, "missed the slot"
        take(k)
        k += 1
    for j in range(6):                               # six pending at once: the engine pipelines them, the rung ends the burst
        put(k + j)
    b.engine_submit(6, flush=True)
    b.engine_wait(k + 6, timeout=8.0)
    for j in range(6):
        take(k + j)
    k += 6
    for _ in range(5):
        put(k)
        b.engine_submit(1, flush=True)
        b.engine_wait(k + 1, timeout=8.0)
        take(k)
        k += 1
    with pytest.raises(gab.GabError):
        b.engine_wait(k + 1, timeout=1.0)              # more than has been published
    with pytest.raises(gab.GabError):
        b.engine_submit(-1)
    assert b.engine_running()
    b.engine_stop()
    assert not b.engine_running()
    for call in (lambda: b.engine_submit(1), lambda: b.engine_feed_one_in_flight(1)):
        with pytest.raises(gab.GabError):              # no running engine
            call()
    assert np.array_equal(bits(host(b.process(dev(xs[k]), mode=gab.CONV_STREAMING))), bits(want[k]))
    a.close()
    b.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_conv_accel_engine_bursts_of_any_shape_walk_one_history(gab, orc, seed):
    """The engine's launch is a sequence of bursts whose boundaries the DOORBELL decides (gab_conv_engine_submit: how many
    buffers, with or without the flush rung, and when) — and workgroups need not even agree on them.  A seeded random
    producer: bursts of 1..9 buffers, flushed or not (a burst without the rung is finished by the next one's), pauses of
    0..3 ms in between, slots reused as soon as their buffer has come back; every output bit for bit what one
    gab_conv_process launch per buffer gives, and ordinary launches continue the stream after the stop."""
    import time
    import torch
    rng = np.random.default_rng(seed)
    T, B, L, R = 64, 512, 4096, 16
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    N = 120
    pre = 2 * seed - 1          # ordinary launches first, an ODD number: the far groups' turns then start on the other pair
    xs = [orc.noise(T * B, seed=7000 + 131 * seed + i) for i in range(pre + N + 1)]
    want = [host(a.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
    for k in range(pre):
        assert np.array_equal(bits(host(b.process(dev(xs[k]), mode=gab.CONV_STREAMING))), bits(want[k]))
    xs, want = xs[pre:], want[pre:]
    side = torch.cuda.Stream()
    in_ring, out_ring = b.engine_start(R, stream=side)
    cur = torch.cuda.current_stream()
    taken = 0

    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()

    def take_until(k_done):
        nonlocal taken
        while taken < k_done:
            h_out.copy_(out_ring[taken % R], non_blocking=True)
            cur.synchronize()
            assert np.array_equal(bits(h_out.numpy()), bits(want[taken])), "buffer %d" % taken
            taken += 1

    published = 0
    while published < N:
        n = int(min(N - published, rng.integers(1, 10)))
        flush = bool(rng.integers(0, 2)) or published + n == N      # the last burst must be finished by somebody
        # slots of this burst must be free: their previous buffers taken
        if published + n - taken > R:
            b.engine_submit(0, flush=True)                           # finish what is pending, then collect it
            b.engine_wait(published, timeout=8.0)
            take_until(published)
        for j in range(n):                                           # copy ENGINES fill the slots: a copy KERNEL may share the engine's
            h_in.copy_(torch.from_numpy(xs[published + j]))           # hardware queue and then waits behind the resident launch
            in_ring[(published + j) % R].copy_(h_in, non_blocking=True)
            cur.synchronize()
        b.engine_submit(n, flush=flush)
        published += n
        if flush and rng.integers(0, 2):
            b.engine_wait(published, timeout=8.0)
            take_until(published)
        time.sleep(float(rng.integers(0, 4)) * 1e-3)
    b.engine_wait(N, timeout=8.0)
    take_until(N)
    b.engine_stop()
    assert np.array_equal(bits(host(b.process(dev(xs[N]), mode=gab.CONV_STREAMING))), bits(want[N]))
    a.close()
    b.close()


def test_conv_accel_engine_feed_matches_batch_launches_and_carries_history(gab, orc):
    """gab_conv_engine_feed on resident rings (what bench.py times): 3 x 16 buffers, one per ring of the doorbell with
    at most eight in flight, leave in the output ring what three batch launches of 16 leave; ordinary launches after
    the stop continue the same stream."""
    import torch
    T, B, L, R = 1024, 512, 4096, 16
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    x = torch.cat([dev(orc.noise(T * B, seed=300 + i)) for i in range(R)])
    side = torch.cuda.Stream()
    in_ring, out_ring = b.engine_rings(R)            # filled BEFORE the launch: at this size the engine holds every CU,
    in_ring.copy_(x.view(R, T * B))                  # and a copy KERNEL would queue behind it (copy engines would not)
    torch.cuda.synchronize()
    b.engine_start(R, stream=side)
    b.engine_feed(3 * R, ahead=8)
    b.engine_stop()
    for _ in range(3):
        y = a.process_batch(x, R)
    torch.cuda.synchronize()
    assert torch.equal(out_ring.reshape(-1).view(torch.int32), y.view(torch.int32))
    x2 = dev(orc.noise(T * B, seed=7))
    assert torch.equal(a.process(x2).view(torch.int32), b.process(x2).view(torch.int32))
    a.close()
    b.close()


def test_conv_accel_engine_refuses_more_channels_than_stay_resident(gab, orc):
    """Every workgroup of the engine waits for words other workgroups write, so all of them must be on the device at
    once: one per compute unit (four channels each).  A plan with more channels is refused at the start — it would
    otherwise stop reporting progress and give up two seconds later."""
    T, B, L = 2048, 512, 4096
    plan = gab.ConvPlan(T, B, L, scheme="split")
    plan.set_ir(dev(orc.conv_accel_ir(L, 8)).repeat(T // 8))
    with pytest.raises(gab.GabError) as e:
        plan.engine_start(8)
    assert "resident" in str(e.value)
    x = dev(orc.noise(T * B, seed=5))
    assert host(plan.process(x)).shape == (T * B,)          # the plan itself is fine
    plan.close()


def test_conv_accel_engine_whose_producer_goes_away_ends_by_itself_and_says_so(gab, orc):
    """The doorbell stops moving (the producer published three buffers WITHOUT the flush rung and left): after the idle
    limit (gab_conv_engine_set_idle_limit, one second here) the resident launch ends by itself, gab_conv_engine_stop
    returns GAB_ERR_RUNTIME and says what the engine consumed — two of the three: the last buffer of a pipelined burst
    waits for its successor — and the plan's history goes on from THERE: no reset, the next ordinary launch continues
    behind buffer 2 bit for bit."""
    import time
    import torch
    T, B, L, R = 64, 512, 4096, 8
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    xs = [dev(orc.noise(T * B, seed=i)) for i in range(R)]
    in_ring, out_ring = b.engine_rings(R)
    in_ring.copy_(torch.cat(xs).view(R, T * B))
    torch.cuda.synchronize()
    with pytest.raises(gab.GabError):
        b.engine_set_idle_limit(0.1)                             # 0.5 .. 3600 s
    b.engine_set_idle_limit(1.0)
    side = torch.cuda.Stream()
    b.engine_start(R, stream=side)
    with pytest.raises(gab.GabError):
        b.engine_set_idle_limit(2.0)                             # taken at the start: not while it runs
    b.engine_publish(3)
    t0 = time.time()
    while b.engine_running() and time.time() - t0 < 20.0:        # the launch must END without a stop (it is on the plan's own stream)
        time.sleep(0.05)
    waited = time.time() - t0
    assert not b.engine_running(), "the engine was still running after %.1f s without a doorbell" % waited
    assert 0.5 < waited < 6.0, waited
    with pytest.raises(gab.GabError) as e:
        b.engine_stop()
    assert "consumed 2 of the 3" in str(e.value), str(e.value)
    assert b.engine_completed() == 2
    want = [a.process(xs[k]) for k in range(3)]
    assert torch.equal(out_ring[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(out_ring[1].view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(b.process(xs[2]).view(torch.int32), want[2].view(torch.int32))     # the history continues behind what was CONSUMED
    x = dev(orc.noise(T * B, seed=77))
    assert torch.equal(a.process(x).view(torch.int32), b.process(x).view(torch.int32))
    a.close()
    b.close()


@pytest.mark.parametrize("T", [64, 1024])
def test_conv_accel_engine_and_keep_warm_exclude_each_other_at_the_call(gab, orc, T):
    """The engine's workgroup fills a compute unit's registers, so keep-warm waves keep it from becoming resident (round 5's
    record: first buffer 484 ms).  The library makes both launches, so it says so at the failing call
    (cuda/bench_base.cu:177-179: errors where they happen): gab_conv_engine_start drops the PLAN'S OWN keep-warm — its first
    buffer, one in flight, then answers in well under a slot and bit for bit — and refuses while a keep-warm object the
    CALLER made is resident; gab_keep_warm_kick refuses to start a launch beside a running engine."""
    import time
    import torch
    B, L, R = 512, 4096, 8
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="classic")
    a.set_ir(ir)
    b.set_ir(ir)
    xs = [orc.noise(T * B, seed=900 + i) for i in range(8)]
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
    b.round_trip_keep_warm(True)
    for k in range(3):                                           # the classic cut's round trips, each ending with a kick
        h_in.copy_(torch.from_numpy(xs[k]))
        b.round_trip(h_in, h_out)
    b.reset()
    b.set_scheme("split")
    want = [host(a.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
    side = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    in_ring, out_ring = b.engine_start(R, stream=side)           # the plan's keep-warm launch was kicked microseconds ago
    h_in.copy_(torch.from_numpy(xs[0]))
    in_ring[0].copy_(h_in, non_blocking=True)
    cur.synchronize()
    t0 = time.perf_counter()
    b.engine_submit(1, flush=True)
    b.engine_wait(1, timeout=8.0)
    first_ms = (time.perf_counter() - t0) * 1e3
    assert first_ms < 5.0, "the engine's first buffer took %.3f ms: something kept its workgroups out" % first_ms
    h_out.copy_(out_ring[0], non_blocking=True)
    cur.synchronize()
    assert np.array_equal(bits(h_out.numpy()), bits(want[0]))
    w = gab.KeepWarm(workgroups=8, idle_seconds=2.0)
    with pytest.raises(gab.GabError) as e:
        w.kick()                                                 # would have to START a launch beside the engine
    assert "engine" in str(e.value)
    assert not w.running()
    b.engine_stop()
    w.kick()
    assert w.running()
    with pytest.raises(gab.GabError) as e:
        b.engine_start(R, stream=side)                           # a keep-warm the CALLER made: refused, not a 0.5 s stall
    assert "gab_keep_warm" in str(e.value), str(e.value)
    assert not b.engine_running()
    w.close()
    in_ring, out_ring = b.engine_start(R, stream=side)           # slots count from 0 again
    for k in (1, 2):
        h_in.copy_(torch.from_numpy(xs[k]))
        in_ring[(k - 1) % R].copy_(h_in, non_blocking=True)
        cur.synchronize()
        b.engine_submit(1, flush=True)
        b.engine_wait(k, timeout=8.0)
        h_out.copy_(out_ring[(k - 1) % R], non_blocking=True)
        cur.synchronize()
        assert np.array_equal(bits(h_out.numpy()), bits(want[k])), "buffer %d" % k
    b.engine_stop()
    a.close()
    b.close()


def test_conv_accel_engine_wait_that_runs_out_says_where_the_launch_is(gab, orc):
    """A wait that runs out names the state of the launch (gab_last_error): here every workgroup is resident and the ONE
    published buffer waits for a successor or the flush rung — the message says so; with the rung it completes."""
    import torch
    T, B, L, R = 64, 512, 4096, 8
    b = gab.ConvPlan(T, B, L, scheme="split")
    b.set_ir(dev(orc.conv_accel_ir(L, T)))
    in_ring, out_ring = b.engine_rings(R)
    in_ring.copy_(torch.cat([dev(orc.noise(T * B, seed=i)) for i in range(R)]).view(R, T * B))
    torch.cuda.synchronize()
    b.engine_start(R, stream=torch.cuda.Stream())
    b.engine_publish(1)
    with pytest.raises(gab.GabError) as e:
        b.engine_wait(1, timeout=0.5)
    assert "every workgroup of the launch is resident" in str(e.value), str(e.value)
    b.engine_submit(0, flush=True)
    b.engine_wait(1, timeout=8.0)
    b.engine_stop()
    b.close()


@pytest.mark.parametrize("T", [64, 1024])
def test_conv_accel_engine_round_trip_from_pinned_host_memory(gab, orc, T):
    """gab_conv_engine_round_trip: the reference's iteration (cuda/bench_base.cu:30-42 around bench_conv1d_accel.cu:258-304)
    through the resident engine — pinned host -> ring slot, doorbell with the flush rung, ring slot -> pinned host, ONE
    buffer in flight — bit for bit one gab_conv_process launch per buffer, more buffers than the ring has slots, and
    refused while something else is in flight."""
    import torch
    B, L, R, N = 512, 4096, 4, 11
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    a.set_ir(ir)
    b.set_ir(ir)
    xs = [orc.noise(T * B, seed=1200 + i) for i in range(N)]
    want = [host(a.process(dev(x), mode=gab.CONV_STREAMING)) for x in xs]
    h_in, h_out = torch.empty(T * B).pin_memory(), torch.empty(T * B).pin_memory()
    with pytest.raises(gab.GabError):
        b.engine_round_trip(h_in, h_out)                         # no running engine
    b.engine_start(R, stream=torch.cuda.Stream())
    for k in range(N):
        h_in.copy_(torch.from_numpy(xs[k]))
        h_out.zero_()
        b.engine_round_trip(h_in, h_out)
        assert np.array_equal(bits(h_out.numpy()), bits(want[k])), "buffer %d" % k
    b.engine_publish(1)                                          # something in flight that nobody waited for
    with pytest.raises(gab.GabError):
        b.engine_round_trip(h_in, h_out)
    b.engine_stop()
    a.close()
    b.close()


@pytest.mark.parametrize("T,B,L,n", [(64, 512, 4096, 11), (1024, 512, 4096, 5), (8, 512, 1500, 9), (5, 512, 2000, 3),
                                      (4, 512, 1100, 37), (2048, 512, 4096, 3), (12, 512, 4096, 1), (36, 512, 3000, 2),
                                      (8192, 512, 4096, 2),      # C5's channel count: 2048 workgroups, eight rounds of the device
                                      (8, 512, 4096, 300),       # more buffers than ONE launch takes (256): the call cuts them into launches

                                      (16, 512, 512, 4), (3, 256, 700, 5)])
def test_conv_accel_batch_equals_one_launch_per_buffer(gab, orc, T, B, L, n):
    """gab_conv_process_batch: n buffers in one launch walk the same history as n launches — same
    bits — including across two batches, mixed with single launches, and for shapes that take other
    kernels.  A plan on the split cut batches with the split cut (conv_split_batch12_kernel: both roles
    of a duo in one resident workgroup) and stays on it; other plans batch with the classic cut."""
    import torch
    ir = dev(orc.conv_accel_ir(L, T))
    b = gab.ConvPlan(T, B, L)
    a = gab.ConvPlan(T, B, L, scheme=b.scheme if B == 512 and L <= 4096 else None)
    a.set_ir(ir)
    b.set_ir(ir)
    scheme = b.scheme
    x = np.concatenate([orc.noise(T * B, seed=60 + i) for i in range(2 * n + 2)])
    seq = np.concatenate([host(a.process(dev(x[i * T * B:(i + 1) * T * B]), mode=gab.CONV_STREAMING))
                          for i in range(2 * n + 2)])
    y1 = host(b.process_batch(dev(x[:n * T * B]), n))
    ym = host(b.process(dev(x[n * T * B:(n + 1) * T * B]), mode=gab.CONV_STREAMING))       # a single launch in between
    y2 = host(b.process_batch(dev(x[(n + 1) * T * B:(2 * n + 1) * T * B]), n))
    yl = host(b.process(dev(x[(2 * n + 1) * T * B:]), mode=gab.CONV_STREAMING))
    assert np.array_equal(bits(seq), bits(np.concatenate([y1, ym, y2, yl])))
    assert b.scheme == scheme                             # a batch call does not change the plan's cut
    with pytest.raises(gab.GabError):
        lib_rc = gab.lib.gab_conv_process_batch(b._h, None, None, 1, None)
        gab.check(lib_rc)
    a.close()
    b.close()


def test_conv_accel_batch_call_longer_than_one_launch_on_the_classic_cut(gab, orc):
    """gab_conv_process_batch cuts a call into launches of at most 256 buffers (a launch's workgroups drift apart over many
    hundred periods): on the classic cut too the 300 buffers of one call are the bits of 300 launches."""
    T, B, L, n = 8, 512, 4096, 300
    ir = dev(orc.conv_accel_ir(L, T))
    a, b = gab.ConvPlan(T, B, L, scheme="classic"), gab.ConvPlan(T, B, L, scheme="classic")
    a.set_ir(ir)
    b.set_ir(ir)
    x = np.concatenate([orc.noise(T * B, seed=500 + i) for i in range(n)])
    seq = np.concatenate([host(a.process(dev(x[i * T * B:(i + 1) * T * B]), mode=gab.CONV_STREAMING)) for i in range(n)])
    assert np.array_equal(bits(seq), bits(host(b.process_batch(dev(x), n))))
    a.close()
    b.close()


def test_conv_accel_split_and_classic_streams_agree(gab, orc):
    """The split cut (far partition every other buffer, one buffer ahead, on its own workgroups)
    and the classic cut are the same convolution: 30 buffers agree to rounding, against each other
    and against the float64 direct form, with a batch call in the middle of both streams and a
    host-io launch at the end; a plan keeps its cut through all of them."""
    import torch
    T, B, L = 64, 512, 4096
    ir = orc.conv_accel_ir(L, T)
    a, b = gab.ConvPlan(T, B, L, scheme="classic"), gab.ConvPlan(T, B, L, scheme="split")
    assert (a.scheme, b.scheme) == ("classic", "split")
    a.set_ir(dev(ir))
    b.set_ir(dev(ir))
    hist = np.zeros(T * L, np.float32)
    xs = [orc.noise(T * B, seed=900 + i) for i in range(30)]
    peak = 0.0
    for i, x in enumerate(xs):
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        peak = max(peak, float(np.abs(ref).max()))
        if i == 20:                                   # two buffers through the batch entry point
            continue
        if i == 21:
            yb = host(b.process_batch(dev(np.concatenate([xs[20], xs[21]])), 2))[T * B:]
            ya = host(a.process_batch(dev(np.concatenate([xs[20], xs[21]])), 2))[T * B:]
        else:
            ya = host(a.process(dev(x), mode=gab.CONV_STREAMING))
            yb = host(b.process(dev(x), mode=gab.CONV_STREAMING))
        if i >= 8:
            assert np.abs(ya - ref).max() <= 1e-5 * peak, i
            assert np.abs(yb - ref).max() <= 1e-5 * peak, i
            assert np.abs(ya - yb).max() <= 2e-6 * peak, i
        assert b.scheme == "split"                                # also after the batch call
    # a host-io launch (pinned buffers) runs the plan's own cut
    hx = torch.from_numpy(xs[0]).pin_memory()
    hy = torch.empty(T * B).pin_memory()
    b.process(hx, out=hy, mode=gab.CONV_STREAMING)
    ya = host(a.process(dev(xs[0]), mode=gab.CONV_STREAMING))
    torch.cuda.synchronize()
    assert b.scheme == "split"
    assert np.abs(hy.numpy() - ya).max() <= 2e-6 * peak
    ya = host(a.process(dev(xs[1]), mode=gab.CONV_STREAMING))
    yb = host(b.process(dev(xs[1]), mode=gab.CONV_STREAMING))
    assert np.abs(ya - yb).max() <= 2e-6 * peak
    # prepared arguments (a loop over a fixed set of buffers) are the same call
    args = b.prepare(dev(xs[0]), torch.empty(T * B, device="cuda"))
    b.launch(args)
    with pytest.raises(gab.GabError):
        b.set_scheme("classic")                       # only on a fresh plan
    b.reset()
    a.reset()
    assert b.scheme == "split"
    y0 = host(b.process(dev(xs[0]), mode=gab.CONV_STREAMING))
    assert peak_err(y0, orc.conv_accel(xs[0], ir, L, B, T)) <= TOL
    with pytest.raises(gab.GabError):
        gab.ConvPlan(6, B, L, scheme="split")         # needs a channel count divisible by 4
    a.close()
    b.close()


def test_conv_accel_long_stream_does_not_drift(gab, orc):
    """400 buffers (the 8-slot ring wraps 50 times; the only carried state is an exact copy of the
    input): the error against the float64 direct form stays where it was after the first window."""
    T, B, L = 4, 512, 4096
    ir = orc.conv_accel_ir(L, T)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    hist = np.zeros(T * L, np.float32)
    errs, peaks = [], []
    for i in range(400):
        x = orc.noise(T * B, seed=2000 + i)
        y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        errs.append(float(np.abs(y - ref).max()))
        peaks.append(float(np.abs(ref).max()))
    peak = max(peaks)
    assert max(errs) <= 1e-5 * peak
    assert max(errs[300:]) <= 1.5 * max(errs[8:100]) + 1e-12        # no growth over the stream
    plan.close()


def test_conv_accel_errors(gab):
    import torch
    with pytest.raises(gab.GabError):
        gab.ConvPlan(0, 512, 512)
    plan = gab.ConvPlan(4, 512, 512)
    with pytest.raises(gab.GabError):                          # IR not set yet
        plan.process(torch.zeros(4 * 512, device="cuda"))
    plan.close()


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", [(128, 512), (7, 1024), (1, 100)])
def test_fft_r2c(gab, orc, T, B):
    x = orc.fft_input(orc.Rand(1), T, B)
    z = host(gab.fft_r2c_1024(dev(x), T)).astype(np.float64)
    tr, ti = orc.fft_truth(x, T)
    tr, ti = tr.reshape(T, 513), ti.reshape(T, 513)
    peak = np.sqrt(tr ** 2 + ti ** 2).max()
    err = (np.abs(z[..., 0] - tr) + np.abs(z[..., 1] - ti)).max()
    assert err / peak <= TOL
    if T <= 16 or (T, B) == (128, 512):
        # the reference golden is ~3e-3 from the truth; we must not be worse
        gr, gi = orc.fft_golden(x, T)
        gerr = (np.abs(gr.reshape(T, 513) - tr) + np.abs(gi.reshape(T, 513) - ti)).max()
        assert err <= gerr
        # and the reference's own gate (|dre|+|dim| <= 1e-3 vs ITS golden) would pass within
        # the golden's own error
        own = (np.abs(z[..., 0] - gr.reshape(T, 513)) + np.abs(z[..., 1] - gi.reshape(T, 513))).max()
        assert own <= gerr + err


def test_modal(gab, orc):
    p = orc.modal_params(4096)
    y = host(gab.modal(dev(p), 4096, 512, 32))
    ref = orc.modal(p, 4096, 512, 32)
    assert peak_err(y, ref) <= 1e-6


# The real bank.  Each mode's phasor sequence is bit-identical to the oracle's
# (same unfused recurrence, same (float)cos/sin((double)angle)); the sums over up to 32 768 modes
# per output sample are taken in a different fixed order, so the gate is the north star's 1e-5,
# relative to the output's peak, against BOTH the fp32 golden and its float64-accumulated twin.
@pytest.mark.parametrize("n_modes,bufsize,tracks", [
    (65536, 512, 32),        # J = 1
    (262144, 512, 32),       # J = 2, 256 workgroups
    (1 << 20, 64, 32),       # the reference size (min(1024*tracks, 2^20)), short buffer
    (4096, 512, 32), (1000, 100, 32),     # ragged: rows and chunks both partial
    (5000, 37, 1), (5000, 48, 2), (5000, 512, 24), (3333, 33, 7), (2048, 16, 64),
    (1, 512, 32), (31, 20, 32),
])
def test_modal_bank_matches_metal_golden(gab, orc, n_modes, bufsize, tracks):
    p = orc.modal_params(n_modes)
    y = host(gab.modal_bank(dev(p), n_modes, bufsize, tracks))
    ref = orc.modal_bank(p, n_modes, bufsize, tracks)
    ref64 = orc.modal_bank_f64acc(p, n_modes, bufsize, tracks)
    peak = np.abs(ref64).max()
    assert np.abs(y - ref64).max() <= 1e-5 * peak
    assert np.abs(y - ref).max() <= 1e-5 * peak
    if n_modes <= tracks:
        # one mode per track: no cross-mode sum at all, so the sequences themselves are compared
        assert np.array_equal(bits(y), bits(ref))


def test_modal_bank_is_reproducible_and_linear_in_amplitude(gab, orc):
    n, B, T = 100000, 128, 32
    p = orc.modal_params(n)
    a = host(gab.modal_bank(dev(p), n, B, T))
    b = host(gab.modal_bank(dev(p), n, B, T))
    assert np.array_equal(bits(a), bits(b))                 # fixed summation order, no atomics
    q = p.copy().reshape(n, 8)
    q[:, 0] *= 2.0                                          # amplitude x2 is exact in fp32
    c = host(gab.modal_bank(dev(q.ravel()), n, B, T))
    assert np.array_equal(bits(c), bits(2.0 * a))
    with pytest.raises(gab.GabError):
        gab.modal_bank(dev(p), n, B, 65)


@pytest.mark.parametrize("variant", ["naive", "accel"])
def test_dwg_delay_lines_bit_exact(gab, orc, variant):
    import torch
    n_wg, B, ML = 128, 512, 2000
    wg, x = orc.dwg_init(n_wg, B)
    v = gab.DWG_NAIVE if variant == "naive" else gab.DWG_ACCEL
    fwd_r = np.zeros(n_wg * ML, np.float32)
    bwd_r = np.zeros(n_wg * ML, np.float32)
    fwd = torch.zeros(n_wg * ML, device="cuda")
    bwd = torch.zeros(n_wg * ML, device="cuda")
    wg_d = dev(wg.view(np.uint8))
    for it in range(3):
        y = host(gab.dwg(wg_d, fwd, bwd, dev(x), B, ML, variant=v))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML)
        assert np.array_equal(bits(y), bits(ry))
        assert np.array_equal(bits(host(fwd)), bits(fwd_r)), "fwd, iteration %d" % it
        assert np.array_equal(bits(host(bwd)), bits(bwd_r)), "bwd, iteration %d" % it
    assert fwd_r.any()


@pytest.mark.parametrize("variant", ["naive", "accel"])
def test_dwg_write_position_late_in_the_line(gab, orc, variant):
    """A write position near the END of a long line: the buffer then visits cells beyond the first
    B of the line (and wraps); input and output taps sit inside that visited range.  Delay lines
    and mix bit-exact over three buffers, for lines shorter and longer than the buffer."""
    import torch
    n_wg, B, ML = 70, 256, 2000
    wg, x = orc.dwg_init(n_wg, B)
    L = wg["length"].astype(np.int64)
    wg["writePos"] = np.where(np.arange(n_wg) % 2 == 0, L - 7, L // 2 + 11) % L
    wg["inputTapPos"] = (wg["writePos"] + 5) % L
    wg["outputTapPos"] = (wg["writePos"] + np.where(np.arange(n_wg) % 3 == 0, 5, 40)) % L
    v = gab.DWG_NAIVE if variant == "naive" else gab.DWG_ACCEL
    fwd_r, bwd_r = np.zeros(n_wg * ML, np.float32), np.zeros(n_wg * ML, np.float32)
    fwd, bwd = torch.zeros(n_wg * ML, device="cuda"), torch.zeros(n_wg * ML, device="cuda")
    for it in range(3):
        y = host(gab.dwg(dev(wg.view(np.uint8)), fwd, bwd, dev(x), B, ML, variant=v))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML)
        assert np.array_equal(bits(y), bits(ry)), it
        assert np.array_equal(bits(host(fwd)), bits(fwd_r)), it
        assert np.array_equal(bits(host(bwd)), bits(bwd_r)), it
    assert np.abs(ry).max() > 0 and fwd_r.any()


@pytest.mark.parametrize("variant", ["naive", "accel"])
def test_dwg_audible_configuration(gab, orc, variant):
    """The reference's tap placement never lets energy reach the output tap
    (SURVEY §8c); move the output tap onto the input tap and start the write
    position mid-line so the ordered mix path is exercised with non-zero data."""
    import torch
    n_wg, B, ML = 37, 300, 2000
    wg, x = orc.dwg_init(n_wg, B)
    wg["outputTapPos"] = wg["inputTapPos"]
    wg["writePos"] = (np.arange(n_wg) * 13) % wg["length"]
    v = gab.DWG_NAIVE if variant == "naive" else gab.DWG_ACCEL
    fwd_r = np.zeros(n_wg * ML, np.float32)
    bwd_r = np.zeros(n_wg * ML, np.float32)
    fwd = torch.zeros(n_wg * ML, device="cuda")
    bwd = torch.zeros(n_wg * ML, device="cuda")
    for it in range(4):
        y = host(gab.dwg(dev(wg.view(np.uint8)), fwd, bwd, dev(x), B, ML, out_tracks=30, variant=v))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=30)
        assert np.array_equal(bits(y), bits(ry))
        assert np.array_equal(bits(host(fwd)), bits(fwd_r))
        assert np.array_equal(bits(host(bwd)), bits(bwd_r))
    assert np.abs(ry).max() > 0


@pytest.mark.parametrize("variant", ["naive", "accel"])
def test_dwg_mix_crowded_and_sparse_samples(gab, orc, variant):
    """The ordered per-sample mix (sparse form, from 2 048 waveguides on): 2 700 waveguides, a third of them with the same short line and the same tap
    phase — their samples collect far more contributions than one wavefront sorts (the scan takes those) — the
    rest spread out (sorted lists of a few entries); samples nobody reaches stay zero.  Bit-exact with the
    golden's waveguide-order sum over four buffers."""
    import torch
    n_wg, B, ML = 2700, 384, 2000
    wg, x = orc.dwg_init(n_wg, B)
    L = wg["length"].astype(np.int64)
    same = np.arange(n_wg) % 3 == 0
    wg["length"] = np.where(same, 96, L)
    L = wg["length"].astype(np.int64)
    wg["writePos"] = np.where(same, 10, (np.arange(n_wg) * 7) % L)
    wg["inputTapPos"] = (wg["writePos"] + 3) % L
    wg["outputTapPos"] = wg["inputTapPos"]
    v = gab.DWG_NAIVE if variant == "naive" else gab.DWG_ACCEL
    fwd_r, bwd_r = np.zeros(n_wg * ML, np.float32), np.zeros(n_wg * ML, np.float32)
    fwd, bwd = torch.zeros(n_wg * ML, device="cuda"), torch.zeros(n_wg * ML, device="cuda")
    for it in range(4):
        y = host(gab.dwg(dev(wg.view(np.uint8)), fwd, bwd, dev(x), B, ML, out_tracks=n_wg, variant=v))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=n_wg)
        assert np.array_equal(bits(y), bits(ry)), it
        assert np.array_equal(bits(host(fwd)), bits(fwd_r)), it
    assert np.abs(ry).max() > 0 and np.count_nonzero(ry) > 10


@pytest.mark.parametrize("n_wg,B,out_tracks", [(8192, 512, 8192), (2048, 2048, 2048), (3000, 100, 2500)])
def test_dwg_large_bank_cells_kernel_appends_to_the_hit_lists(gab, orc, n_wg, B, out_tracks):
    """Banks from 2 048 mixed waveguides on: the cells kernel's tap threads append to their samples' lists themselves
    (dwg_cells_append_kernel; no gather launch), the mix kernel sorts and adds the lists in waveguide order and puts the
    counters back to zero.  8 192 lines (the size the per-size
    table prices), the longest buffer the staged input holds, and a mix over fewer tracks than there are lines — with
    taps that are really reached (the reference's placement never is: SURVEY 8c) and write positions spread over the
    lines; delay lines and mix bit-exact over four buffers on one workspace, then two calls on two streams at once (a
    counter slot each)."""
    import torch
    ML = 2000
    wg, x = orc.dwg_init(n_wg, B)
    L = wg["length"].astype(np.int64)
    wg["writePos"] = (np.arange(n_wg) * 13) % L
    wg["outputTapPos"] = wg["inputTapPos"] = (wg["writePos"] + (np.arange(n_wg) % 5) * 3) % L
    fwd_r, bwd_r = np.zeros(n_wg * ML, np.float32), np.zeros(n_wg * ML, np.float32)
    fwd, bwd = torch.zeros(n_wg * ML, device="cuda"), torch.zeros(n_wg * ML, device="cuda")
    wg_d = dev(wg.view(np.uint8))
    for it in range(4):
        y = host(gab.dwg(wg_d, fwd, bwd, dev(x), B, ML, out_tracks=out_tracks, variant=gab.DWG_ACCEL))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=out_tracks)
        assert np.array_equal(bits(y), bits(ry)), it
        assert np.array_equal(bits(host(fwd)), bits(fwd_r)), it
        assert np.array_equal(bits(host(bwd)), bits(bwd_r)), it
    assert np.abs(ry).max() > 0 and np.count_nonzero(ry) >= 3
    # two launches in flight on two streams: same state in, same bits out, twice
    f2, b2 = fwd.clone(), bwd.clone()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        y1 = gab.dwg(wg_d, fwd, bwd, dev(x), B, ML, out_tracks=out_tracks, variant=gab.DWG_ACCEL)
    with torch.cuda.stream(s2):
        y2 = gab.dwg(wg_d, f2, b2, dev(x), B, ML, out_tracks=out_tracks, variant=gab.DWG_ACCEL)
    torch.cuda.synchronize()
    ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=out_tracks)
    assert np.array_equal(bits(host(y1)), bits(ry)) and np.array_equal(bits(host(y2)), bits(ry))
    assert np.array_equal(bits(host(f2)), bits(fwd_r))


@pytest.mark.parametrize("n,T,B,samples", [(20, 4, 16, 16), (52, 128, 512, 24), (33, 3, 8, 8),
                                          (128, 16, 8, 6),       # C4's grid, a few samples (the resident kernel; in step form 32 x 16 tiles)
                                          (100, 3, 6, 6),        # resident too (in step form 32 x 8 tiles with a partial last tile row)
                                          (148, 2, 4, 4)])       # past the resident kernel's 128: 64 x 8 tiles
def test_fdtd_bit_exact(gab, orc, n, T, B, samples):
    import torch
    P = orc.fdtd_params(n)
    G = gab.fdtd_default_params(n)
    for a, b in (("src_x", "source_x"), ("src_y", "source_y"), ("src_z", "source_z"),
                 ("rcv_x", "receiver_x"), ("rcv_y", "receiver_y"), ("rcv_z", "receiver_z")):
        assert getattr(P, a) == getattr(G, b)
    assert P.dt_over_rho_dx == G.dt_over_rho_dx and P.rho_c2_dt_over_dx == G.rho_c2_dt_over_dx
    if n == 52:
        assert (G.source_x, G.source_y, G.source_z) == (25, 25, 5)     # bench_fdtd3d.cuh:27-33
        assert (G.receiver_x, G.receiver_y, G.receiver_z) == (40, 15, 25)
    x = orc.Rand(1).bipolar(T * B)
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    plan = gab.FdtdPlan(G)
    # rooms up to 128 cells wide whose fields fit the LDS take the resident whole-buffer kernel
    assert plan.resident()[0] == (n <= 128)
    out = torch.zeros(T * B, device="cuda")
    half = samples // 2
    for first, cnt in ((0, half), (half, samples - half)):       # state carries across calls
        orc.fdtd(P, grids, x, ref, T, B, first, cnt, fused=True)
        plan.process(dev(x), out, T, B, first, cnt)
    assert np.array_equal(bits(host(out)), bits(ref))
    assert np.array_equal(bits(host(plan.pressure()).ravel()), bits(grids[0]))
    assert np.abs(grids[0]).max() > 0
    plan.reset()
    assert not host(plan.pressure()).any()
    plan.close()


@pytest.mark.parametrize("dims", [(8, 6, 5), (24, 21, 19), (64, 30, 9), (128, 5, 7), (12, 64, 64), (128, 40, 50),
                                  (50, 21, 19), (7, 9, 11), (127, 6, 5), (5, 4, 4), (33, 40, 12)])    # rows that end in a part quad
def test_fdtd_resident_rooms(gab, orc, dims):
    """The LDS-resident kernel on rooms that are not cubes: blocks that do not divide the room (a clipped last
    block in y and in z), one-quad and full-width rows, rows that are no multiple of four cells (the last quad
    is partly padding), more workgroups along one axis than the other; several
    calls in a row (the exchange tags go on across launches), a reset in between, source and receiver placed by
    the reference's proportions.  Bit for bit the oracle's fields and outputs."""
    import torch
    nx, ny, nz = dims
    P = orc.fdtd_params(nx, ny, nz)
    G = gab.fdtd_default_params(nx, ny, nz)
    T, B = 3, 10
    plan = gab.FdtdPlan(G)
    is_resident, workgroups = plan.resident()
    assert is_resident and 2 <= workgroups <= torch.cuda.get_device_properties(0).multi_processor_count
    for rnd in range(2):
        x = orc.Rand(7 + rnd).bipolar(T * B)
        grids = orc.fdtd_grids(P)
        ref = np.zeros(T * B, np.float32)
        out = torch.zeros(T * B, device="cuda")
        for first, cnt in ((0, 1), (1, 6), (7, 3)):
            orc.fdtd(P, grids, x, ref, T, B, first, cnt, fused=True)
            plan.process(dev(x), out, T, B, first, cnt)
        assert np.array_equal(bits(host(out)), bits(ref))
        assert np.array_equal(bits(host(plan.pressure()).ravel()), bits(grids[0]))
        assert np.abs(grids[0]).max() > 0
        plan.reset()
    plan.close()


def test_fdtd_resident_launches_from_two_streams(gab, orc):
    """Two plans whose resident launches each want (nearly) every CU, driven from two streams with no host
    sync in between: the library chains resident launches on a device, so neither waits for workgroups the other
    is keeping off the chip (which would end in the one-second poll timeout and an error)."""
    import torch
    n, T, B = 64, 2, 6
    P, G = orc.fdtd_params(n), gab.fdtd_default_params(n)
    x = orc.Rand(3).bipolar(T * B)
    xd = dev(x)
    plans = [gab.FdtdPlan(G), gab.FdtdPlan(G)]
    assert all(p.resident()[0] for p in plans)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(T * B, device="cuda") for _ in plans]
    torch.cuda.synchronize()
    for first, cnt in ((0, 2), (2, 1), (3, 3)):
        for p, st, o in zip(plans, streams, outs):
            with torch.cuda.stream(st):
                p.process(xd, o, T, B, first, cnt)
    torch.cuda.synchronize()
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    for p, o in zip(plans, outs):
        assert np.array_equal(bits(host(o)), bits(ref))
        assert np.array_equal(bits(host(p.pressure()).ravel()), bits(grids[0]))
        p.close()


def test_fdtd_resident_beside_other_work(gab, orc):
    """Uneven load: another stream streams half a gigabyte through the chip over and over while the resident
    kernel runs, so its workgroups start at different times and wait for neighbours that are not on a CU yet.
    The hand-off must deliver every word regardless (granule tags, bounded polls): bit-exact fields and output."""
    import torch
    n, T, B = 64, 2, 24
    P, G = orc.fdtd_params(n), gab.fdtd_default_params(n)
    x = orc.Rand(5).bipolar(T * B)
    xd = dev(x)
    plan = gab.FdtdPlan(G)
    assert plan.resident()[0]
    out = torch.zeros(T * B, device="cuda")
    big = torch.ones(128 * 1024 * 1024, device="cuda")          # 512 MB
    hog, work = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(hog):
        for _ in range(60):
            big.mul_(1.0000001)
    with torch.cuda.stream(work):
        for first, cnt in ((0, 8), (8, 8), (16, 8)):
            plan.process(xd, out, T, B, first, cnt)
    with torch.cuda.stream(hog):
        for _ in range(20):
            big.mul_(1.0000001)
    torch.cuda.synchronize()
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    assert np.array_equal(bits(host(out)), bits(ref))
    assert np.array_equal(bits(host(plan.pressure()).ravel()), bits(grids[0]))
    plan.close()


def test_fdtd_c4_grid_scaling_property(gab, orc):
    """BASELINE C4 (128^3): every operation of the scheme is linear and a factor 2 is exact in
    fp32, so doubling the input must double every output bit for bit, at full size."""
    import torch
    n, T, B = 128, 16, 32
    x = orc.Rand(1).bipolar(T * B)
    fields = []
    for scale in (1.0, 2.0):
        plan = gab.FdtdPlan(gab.fdtd_default_params(n))
        out = torch.zeros(T * B, device="cuda")
        plan.process(dev((x * np.float32(scale)).astype(np.float32)), out, T, B, 0, B)
        # 96 steps move the wave ~28 cells: it has not reached the receiver, so the field is compared
        fields.append(host(plan.pressure()).ravel())
        plan.close()
    assert np.count_nonzero(fields[0]) > 10000
    # exact wherever the values are normal numbers; the numerical precursor of the front runs
    # through the subnormal range, where x and 2x do not round alike
    # (products like c1 * dp go subnormal there and their lost bits reach values up to ~1e-27)
    normal = np.abs(fields[0]) > 1e-20
    assert np.count_nonzero(normal) > 10000
    assert np.array_equal(bits(fields[1][normal]), bits(np.float32(2.0) * fields[0][normal]))
    assert np.abs(fields[1][~normal] - 2.0 * fields[0][~normal]).max() < 1e-25


@pytest.mark.parametrize("n,cuts,T,B", [
    (20, [(0, 10), (10, 20)], 4, 12),                 # scalar rows; even cut
    (52, [(0, 5), (5, 6), (6, 26), (26, 52)], 8, 10), # source plane z=5 is a one-plane slab of its own
    (52, [(0, 25), (25, 52)], 8, 40),                 # receiver plane z=25 sits on a cut; the wave crosses it
    (33, [(0, 1), (1, 32), (32, 33)], 3, 6),          # the two boundary planes alone; odd row length
    (128, [(0, 40), (40, 90), (90, 128)], 4, 4),      # C4's grid, LDS-halo kernel, uneven thirds
])
def test_fdtd_z_slabs_reproduce_the_single_grid(gab, orc, n, cuts, T, B):
    """any cut of the room into z-slabs with plane exchange gives the single grid's
    output and pressure field bit for bit (and therefore the oracle's)."""
    import torch
    from gpuaudiobench_amd import fdtd_slabs as fs
    G = gab.fdtd_default_params(n)
    x = orc.Rand(3).bipolar(T * B)
    P = orc.fdtd_params(n)
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)

    slabs = [fs.FdtdSlab(G, a, b) for a, b in cuts]
    assert sum(s.owns_source for s in slabs) == 1 and sum(s.owns_receiver for s in slabs) == 1
    out = torch.zeros(T * B, device="cuda")
    fs.process_local(slabs, dev(x), out, T, B)
    field = torch.cat([s.pressure() for s in slabs]).cpu().numpy().ravel()
    assert np.array_equal(bits(host(out)), bits(ref))
    assert np.array_equal(bits(field), bits(grids[0]))
    assert np.abs(grids[0]).max() > 0
    if B >= 40:
        assert np.abs(ref).max() > 0                  # the front reached the receiver through the cut

    # a second buffer: slab state carries on like the plan's
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    fs.process_local(slabs, dev(x), out, T, B)
    assert np.array_equal(bits(host(out)), bits(ref))
    for s in slabs:
        s.reset()
        assert not s.pressure().any()
        s.close()


@pytest.mark.parametrize("n,T,B", [(20, 5, 10), (52, 12, 24), (128, 6, 4)])
def test_fdtd_track_dependent_positions(gab, orc, n, T, B):
    """SURVEY 8f-4, second half: every track with its own source and receiver cell (the Metal
    port's 'can be made track-dependent later'), bit-exact against the oracle — including
    tracks that share a source cell (summed in track order), a receiver that is also a source,
    and cells on the damped boundary shell."""
    import torch
    G = gab.fdtd_default_params(n)
    rng = np.random.RandomState(n)
    src = rng.randint(1, n - 1, size=(T, 3)).astype(np.int32)
    rcv = rng.randint(1, n - 1, size=(T, 3)).astype(np.int32)
    src[1] = src[0]                                   # two tracks, one source cell
    src[T - 1] = src[0]                               # ... and a third, not adjacent in track order
    rcv[2] = src[3]                                   # a receiver on another track's source
    rcv[0] = src[0] + np.array([1, 0, 0], np.int32)   # right next to a source: heard within a step
    src[4] = (0, n // 2, n // 2)                      # on the boundary shell
    x = orc.Rand(9).bipolar(T * B)
    P = orc.fdtd_params(n)
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    plan = gab.FdtdPlan(G)
    plan.set_track_positions(src, rcv)
    out = torch.zeros(T * B, device="cuda")
    half = B // 2
    for first, cnt in ((0, half), (half, B - half)):
        orc.fdtd_tracks(P, grids, x, ref, T, B, first, cnt, src, rcv, fused=True)
        plan.process(dev(x), out, T, B, first, cnt)
    assert np.array_equal(bits(host(out)), bits(ref))
    assert np.array_equal(bits(host(plan.pressure()).ravel()), bits(grids[0]))
    got = host(out).reshape(T, B)
    assert np.abs(got[0]).max() > 0 and not np.array_equal(got[0], got[1])     # tracks hear different things
    with pytest.raises(gab.GabError):
        plan.process(dev(x), out, T + 1, B, 0, 1)     # positions were given for T tracks
    with pytest.raises(gab.GabError):
        bad = src.copy()
        bad[0, 0] = n
        plan.set_track_positions(bad, rcv)
    # back to the shared cells: the plan behaves like a fresh one
    plan.set_track_positions(None, None)
    plan.reset()
    grids = orc.fdtd_grids(P)
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    plan.process(dev(x), out, T, B, 0, B)
    assert np.array_equal(bits(host(out)), bits(ref))
    plan.close()


def test_fdtd_slab_argument_errors(gab):
    import ctypes as C
    import torch
    from gpuaudiobench_amd import fdtd_slabs as fs
    G = gab.fdtd_default_params(20)
    for a, b in ((-1, 5), (5, 5), (7, 3), (0, 21)):
        with pytest.raises(gab.GabError):
            fs.FdtdSlab(G, a, b)
    s = fs.FdtdSlab(G, 0, 10)
    with pytest.raises(gab.GabError):
        s.inject(0)                                   # no source sums yet
    x = torch.zeros(16, device="cuda")
    with pytest.raises(gab.GabError):                 # the whole-grid entry point refuses a slab
        gab.check(gab.lib.gab_fdtd_process(s._h, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                           2, 8, 0, 8, None))
    assert fs.slab_ranges(10, 3) == [(0, 4), (4, 7), (7, 10)]
    with pytest.raises(ValueError):
        fs.slab_ranges(3, 4)
    s.close()


@pytest.mark.parametrize("T,B", [(130, 512), (1024, 512), (512, 200), (4096, 64), (2048, 1000)])
def test_rndmem_small_pool(gab, orc, T, B):
    """Track counts whose tile count is a multiple of eight walk the grid XCD-locally (rndmem_kernel);
    the others in plain order: both bit-exact, over three buffers of advancing playheads."""
    N = 1 << 20
    pool = orc.rndmem_pool(N)
    ph, st, en = orc.rndmem_playheads(T, B, pool_elems=N)
    pd = dev(pool)
    for it in range(3):
        y = host(gab.rndmem(pd, dev(ph), T, B))
        assert np.array_equal(bits(y), bits(orc.rndmem(pool, ph, B)))
        orc.rndmem_advance(ph, st, en, B)


def test_rndmem_reference_pool_512mib(gab, orc):
    T, B = 128, 512
    pool = orc.rndmem_pool()
    ph, st, en = orc.rndmem_playheads(T, B)
    y = host(gab.rndmem(dev(pool), dev(ph), T, B))
    assert orc.fnv_survey(y) == "b59ca490d48ee02c"               # SURVEY §8c pin
    assert np.array_equal(bits(y), bits(orc.rndmem(pool, ph, B)))


# ---------------------------------------------------------------- seeded random shapes
def _rng_shapes(seed, n, lo, hi):
    r = np.random.RandomState(seed)
    return [tuple(int(v) for v in r.randint(lo, hi, size=len(lo))) for _ in range(n)]


@pytest.mark.parametrize("T,B", _rng_shapes(11, 6, (1, 1), (300, 700)))
def test_random_shapes_gainstats_and_iir(gab, orc, T, B):
    import torch
    x = orc.noise(T * B, seed=T * 1000 + B)
    out, stats = gab.gainstats(dev(x), T, B, 0.5)
    ro, rs = orc.gainstats(x, T, B)
    assert np.array_equal(bits(host(out)), bits(ro))
    assert np.array_equal(host(stats)[1::2], rs[1::2])                       # max: exact
    assert np.abs(host(stats)[0::2] - rs[0::2]).max() <= 1e-5                # mean: order-dependent sum
    c = orc.iir_coeffs(0.25)
    st_g = torch.zeros(2 * T, device="cuda")
    st_o = np.zeros(2 * T, np.float32)
    for k in range(2):
        xk = orc.noise(T * B, seed=k + 5)
        yg = host(gab.iir(dev(xk), dev(c), st_g, T, B, sequential=True))
        yo = orc.iir(xk, c, st_o, T, B)
        assert np.array_equal(bits(yg), bits(yo))
    assert np.array_equal(bits(host(st_g)), bits(st_o))


@pytest.mark.parametrize("T,L,nbuf", _rng_shapes(23, 5, (1, 513, 2), (40, 4097, 6)))
def test_random_shapes_streaming_convolution(gab, orc, T, L, nbuf):
    """Fused path (B = 512) at random channel counts and tap counts in (512, 4096]."""
    B = 512
    ir = orc.conv_accel_ir(L, T)
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(dev(ir))
    hist = np.zeros(T * L, np.float32)
    peak, worst = 0.0, 0.0
    for i in range(nbuf + 8):
        x = orc.noise(T * B, seed=900 + i)
        y = host(plan.process(dev(x), mode=gab.CONV_STREAMING))
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        peak = max(peak, float(np.abs(ref).max()))
        worst = max(worst, float(np.abs(y - ref).max()))
    assert worst <= 1e-5 * peak
    plan.close()


@pytest.mark.parametrize("T,B", _rng_shapes(37, 4, (1, 8), (200, 600)))
def test_random_shapes_rndmem_and_modal_bank(gab, orc, T, B):
    N = 1 << 18
    pool = orc.rndmem_pool(N)
    r = np.random.RandomState(T * 7 + B)
    ph = r.randint(0, N - B, size=T).astype(np.int32)
    y = host(gab.rndmem(dev(pool), torch_i32(ph), T, B))
    assert np.array_equal(bits(y), bits(orc.rndmem(pool, ph, B)))
    tracks = 1 + (T % 32)
    nm = 37 * T + 5
    p = orc.modal_params(nm)
    yb = host(gab.modal_bank(dev(p), nm, B, tracks))
    ref = orc.modal_bank_f64acc(p, nm, B, tracks)
    assert np.abs(yb - ref).max() <= 1e-5 * np.abs(ref).max()


def torch_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def test_plans_release_their_device_memory(gab):
    """Every plan frees what it allocated (spectra, history ring, FDTD fields, cached graphs):
    free device memory is back where it started after many create / use / close cycles."""
    import torch
    T, B, L = 256, 512, 4096
    ir = torch.from_numpy(gab.harness.conv_accel_ir(L, T)).cuda()
    x = torch.from_numpy(gab.harness.noise(T * B)).cuda()
    xf = torch.from_numpy(gab.harness.noise(4 * 16)).cuda()
    out = torch.empty(T * B, device="cuda")
    outf = torch.empty(4 * 16, device="cuda")

    def cycle():
        plan = gab.ConvPlan(T, B, L)
        plan.set_ir(ir)
        plan.process(x, out=out)
        plan.close()
        f = gab.FdtdPlan(gab.fdtd_default_params(64))
        f.process(xf, outf, 4, 16, 0, 16)                 # 51 launches: goes through a captured graph
        f.close()
        from gpuaudiobench_amd import fdtd_slabs as fs
        slabs = [fs.FdtdSlab(gab.fdtd_default_params(32), a, b) for a, b in fs.slab_ranges(32, 2)]
        fs.process_local(slabs, xf, outf, 4, 16)
        for s in slabs:
            s.close()

    cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (8 << 20), (free0, free1)      # one cycle allocates > 60 MiB
