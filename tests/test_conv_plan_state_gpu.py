"""The conv plan when its state changes partway through a stream, on every route gab_conv_create / _create_scheme
picks: a stateless call in the middle of a stream, reset after the history has wrapped, set_ir at an even and an odd
buffer (per-buffer launches and between batch launches), and the hand-offs between streams (a reset or set_ir on one
stream while a launch on another is still queued).  The float64 reference is the whole-stream convolution with the
response in force at each buffer (test_conv_fdl_host.stream_reference with a schedule).

The contract these hold the plan to (gab_conv_set_ir): new taps from the next buffer on, bit-identical to a plan that
had them from the start; the split cut's first buffer after the switch is equal to rounding only (see
test_set_ir_mid_stream)."""
import math

import numpy as np
import pytest

from test_conv_fdl_host import stream_reference

pytestmark = pytest.mark.gpu

TOL = 1e-5              # against float64, of the stream's peak
SPLIT_TOL = 2e-6        # split cut against the classic cut, of the stream's peak (test_gpu_parity.py)
# torch.cuda._sleep spins for this many clock64() ticks.  Measured on an MI355X with events around the sleep: 5e7 ticks
# = 20.86 ms (1e7 = 4.18 ms), so this holds a stream for ~50 ms: long enough that every later call of a hand-off case
# is queued while the hold still runs (each case asserts that), short enough that the ~55 cases cost a few seconds.
HOLD_CYCLES = 120_000_000

# route id -> (tracks, bufsize, ir_len, scheme argument, scheme reported, kind)
ROUTES = {
    "classic-T6": (6, 512, 4096, None, "classic", "classic"),
    "classic-T8": (8, 512, 4096, "classic", "classic", "bank"),
    "split": (8, 512, 4096, None, "split", "split"),
    "fused-notail": (5, 512, 512, None, "classic", "fused"),
    "classic-tail1000": (8, 512, 1000, None, "classic", "classic"),
    "uniform-256": (3, 256, 3000, None, "classic", "uniform"),
    "uniform-1024": (2, 1024, 16384, None, "classic", "uniform"),
    "uniform-32": (3, 32, 700, None, "classic", "uniform"),
    "direct": (3, 300, 700, None, "classic", "direct"),
    "fdl": (4, 512, 20000, "fdl", "fdl", "fdl"),
    "fdl-groups": (6, 128, 5000, "fdl", "fdl", "fdl"),
}
FDL_CHUNK = 16          # buffers per fdl batch launch (k_conv_fdl.hip): its delay line holds K + 15 spectra


def _uniform_layout(B, L):
    S = 4096 - B
    J = 1 + (-(-(L - B) // S) if L > B else 0)
    need = 4096 + B + (B + (J - 2) * S if J > 1 else 0)
    ring = 4096
    while ring < need:
        ring *= 2
    return J, ring


def expected_state_bytes(T, B, L, kind):
    """(spectra, history) of gab_conv_state_bytes for the route: proves which one the plan took."""
    pairs = (T + 1) // 2
    a, b = 16 * pairs * 513, 16 * pairs * 2049          # float4 (P, M) per bin: 1024- and 4096-point banks
    ring8 = 4 * pairs * 2 * 8 * 512                     # the fused cuts' history: 8 blocks of 512, channels paired
    if kind == "fused":
        return a, ring8
    if kind == "classic":
        return a + b, ring8
    if kind in ("split", "bank"):                       # both cuts' spectra and the split cut's 4-slot carry ring
        return 2 * (a + b), ring8 + 8 * pairs * 4 * 512
    if kind == "uniform":
        J, ring = _uniform_layout(B, L)
        return 16 * J * pairs * 2049, 8 * pairs * ring
    if kind == "direct":
        hlen = max(1, -(-(L - 1) // B)) * B
        return 4 * T * L, 4 * T * hlen
    K = math.ceil(L / B)
    return 8 * K * T * (B + 1), 8 * (K + FDL_CHUNK - 1) * T * (B + 1) + 4 * T * B


def wrap_len(T, B, L, kind):
    """Buffers until the route's history ring (or delay line) has been overwritten once."""
    if kind in ("classic", "bank", "split", "fused"):
        return 8
    if kind == "uniform":
        return _uniform_layout(B, L)[1] // B
    if kind == "direct":
        return max(1, -(-(L - 1) // B))
    return math.ceil(L / B) + FDL_CHUNK - 1


def fill_len(B, L):
    """Buffers until every tap sees real input."""
    return math.ceil(L / B)


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


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def reverb_ir(T, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, L)) * np.exp(-np.arange(L) / max(L / 5.0, 1.0))).astype(np.float32).ravel()


def inputs(T, B, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(T * B).astype(np.float32) for _ in range(n)]


@pytest.fixture
def make(gab):
    """make(route, ir[, scheme]): a plan with its taps set, closed when the test ends, passed or failed.  (A plan left
    to the garbage collector is destroyed with a device-wide sync wherever the collector runs: inside a later
    hand-off case that sync would wait out the hold.)"""
    made = []

    def plan(route, ir, scheme=None):
        T, B, L, arg, _, _ = ROUTES[route]
        p = gab.ConvPlan(T, B, L, scheme=scheme or arg)
        made.append(p)
        p.set_ir(dev(ir))
        return p
    yield plan
    for p in made:
        p.close()


def run_stream(plan, xs):
    return [host(plan.process(dev(x))) for x in xs]


@pytest.fixture(params=list(ROUTES))
def route(request, gab):
    """Each case first proves the route it names: the scheme the plan reports and its state's size."""
    name = request.param
    T, B, L, arg, scheme, kind = ROUTES[name]
    p = gab.ConvPlan(T, B, L, scheme=arg)
    assert p.scheme == scheme
    assert tuple(p.state_bytes()) == expected_state_bytes(T, B, L, kind), name
    return name


def shape(route):
    T, B, L, _, _, kind = ROUTES[route]
    return T, B, L, kind


# (a) ----------------------------------------------------------------------------------------------------------------
def test_stateless_calls_mid_stream(gab, make, orc, route):
    """A stateless call every third buffer matches the golden (the first buffer from zero history) and leaves the
    stream alone: the streaming outputs are those of an uninterrupted twin, bit for bit, past a wrap of the ring."""
    T, B, L, kind = shape(route)
    ir = reverb_ir(T, L, seed=1)
    n = wrap_len(T, B, L, kind) + fill_len(B, L) + 4
    xs, zs = inputs(T, B, n, seed=2), inputs(T, B, n, seed=3)
    a, b = make(route, ir), make(route, ir)
    ya = run_stream(a, xs)
    for i, x in enumerate(xs):
        if i % 3 == 0:
            ys = host(b.process(dev(zs[i]), mode=gab.CONV_STATELESS))
            g = orc.conv_accel(zs[i], ir, L, B, T)
            assert np.abs(ys - g).max() <= TOL * np.abs(g).max(), i
        assert same_bits(host(b.process(dev(x))), ya[i]), i


# (b) ----------------------------------------------------------------------------------------------------------------
def test_reset_after_the_ring_has_wrapped_is_a_fresh_plan(gab, make, route):
    T, B, L, kind = shape(route)
    ir = reverb_ir(T, L, seed=4)
    w = wrap_len(T, B, L, kind)
    xs, xs2 = inputs(T, B, w + 3, seed=5), inputs(T, B, w + 2, seed=6)
    a, fresh = make(route, ir), make(route, ir)
    run_stream(a, xs)
    a.reset()
    for i, x in enumerate(xs2):
        assert same_bits(host(a.process(dev(x))), host(fresh.process(dev(x)))), i


# (c) ----------------------------------------------------------------------------------------------------------------
def switch_points(B, L):
    m0 = max(fill_len(B, L), 8)
    return {"even": m0 + (m0 & 1), "odd": m0 + 1 - (m0 & 1)}


@pytest.mark.parametrize("parity", ["even", "odd"])
def test_set_ir_mid_stream(gab, make, route, parity):
    """set_ir(ir2) before buffer m (m past the history's fill, even and odd): from m on the outputs follow the switched
    float64 reference, and they are the bits of a plan that had ir2 from the start and saw the same inputs.

    The split cut computes its far share (taps [1024, 4096)) one buffer ahead: F of block k, for one channel pair in
    two (alternating with k), parks blocks k+1 and k+2 in the carry ring.  At the switch the ring holds the far share
    of blocks m and m+1 under the old taps; set_ir recomputes both as F of block m-1 over the history ring.  For the
    pairs whose F ran at m-1 that is the twin's carry bit for bit; for the others the twin's block m came from F of
    block m-2 (another window: equal to rounding) and its block m+1 from F of block m, as here.  So buffer m is held
    to the split-against-classic bound, and from buffer m+1 on the outputs are the split twin's bits."""
    T, B, L, kind = shape(route)
    m = switch_points(B, L)[parity]
    n = m + wrap_len(T, B, L, kind) + 4
    ir1, ir2 = reverb_ir(T, L, seed=7), reverb_ir(T, L, seed=8)
    xs = inputs(T, B, n, seed=9 + m)
    refs = stream_reference(xs, [(0, ir1), (m, ir2)], T, B, L)
    peak = max(np.abs(r).max() for r in refs)
    a, twin = make(route, ir1), make(route, ir2)
    ys = run_stream(a, xs[:m])
    yt = run_stream(twin, xs[:m])
    a.set_ir(dev(ir2))
    ys += run_stream(a, xs[m:])
    yt += run_stream(twin, xs[m:])
    errs = [np.abs(y - r).max() / peak for y, r in zip(ys, refs)]
    assert max(errs) <= TOL, (int(np.argmax(errs)), max(errs))
    exact_from = m
    if kind == "split":
        classic = make(route, ir2, scheme="classic")
        yc = run_stream(classic, xs[:m + 1])
        assert np.abs(ys[m] - yc[m]).max() <= SPLIT_TOL * peak
        exact_from = m + 1
    for i in range(exact_from, n):
        assert same_bits(ys[i], yt[i]), i


# (d) ----------------------------------------------------------------------------------------------------------------
def test_set_ir_between_batch_calls(gab, make, route):
    """process_batch(n), set_ir, process_batch(n): the bits of per-buffer launches with the same switch, and the
    switched reference.  n = 9 on the fused cuts (the split and classic batch kernels; the switch lands on an odd
    buffer), 20 on fdl (a batch spans two of its 16-buffer chunks); other routes take the batch one buffer at a time."""
    T, B, L, kind = shape(route)
    n = 20 if kind == "fdl" else 9
    before = -(-fill_len(B, L) // n)                     # batches before the switch: the history has filled
    m, total = before * n, (before + 2) * n
    ir1, ir2 = reverb_ir(T, L, seed=10), reverb_ir(T, L, seed=11)
    xs = inputs(T, B, total, seed=12)
    refs = stream_reference(xs, [(0, ir1), (m, ir2)], T, B, L)
    peak = max(np.abs(r).max() for r in refs)
    a, b, twin = make(route, ir1), make(route, ir1), make(route, ir2)
    ya = []
    for k in range(before + 2):
        if k == before:
            a.set_ir(dev(ir2))
        ya += list(host(a.process_batch(dev(np.concatenate(xs[k * n:(k + 1) * n])), n)).reshape(n, T * B))
    yb = run_stream(b, xs[:m])
    b.set_ir(dev(ir2))
    yb += run_stream(b, xs[m:])
    yt = run_stream(twin, xs)
    for i in range(total):
        assert same_bits(ya[i], yb[i]), i
    errs = [np.abs(y - r).max() / peak for y, r in zip(ya, refs)]
    assert max(errs) <= TOL, (int(np.argmax(errs)), max(errs))
    for i in range(m + (kind == "split"), total):
        assert same_bits(ya[i], yt[i]), i


# (e) ----------------------------------------------------------------------------------------------------------------
def held_stream():
    """A stream at the highest priority.  The runtime maps streams onto a few hardware queues per priority: a stream
    that shared the held one's queue would stand behind the hold whatever the plan orders, and hide a missing wait.
    The other streams of these cases (the default one, new ones) are at normal priority."""
    import torch
    return torch.cuda.Stream(priority=-1)


def hold(stream):
    """Queues a spin of HOLD_CYCLES on `stream`; returns an event behind it (query() is False while it runs)."""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(HOLD_CYCLES)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def staged(xs):
    """Inputs and outputs allocated before a hold: an upload from pageable memory waits for its stream, and so would
    the host; nothing between the hold and the checks allocates."""
    import torch
    return [dev(x) for x in xs], dev(np.concatenate(xs)), torch.empty(len(xs) * xs[0].size, device="cuda")


def launch(plan, ins, form):
    """The staged buffers through `plan` on the current stream, without a host sync: one launch each or one batch."""
    each, whole, out = ins
    if form == "process":
        outs = out.view(len(each), -1)
        for x, o in zip(each, outs):
            plan.process(x, out=o)
    else:
        plan.process_batch(whole, len(each), out=out)
    return out


HELD = "the hold had ended before the later call was queued: the case proves nothing (raise HOLD_CYCLES)"


@pytest.mark.parametrize("form", ["process", "batch"])
def test_reset_on_a_held_stream_then_launch_on_another(gab, make, route, form):
    """(e1) reset on stream A behind a hold, then launches on stream B with no host sync: B waits for the reset and
    gives a fresh plan's bits."""
    import torch
    T, B, L, kind = shape(route)
    ir = reverb_ir(T, L, seed=13)
    xs, xs2 = inputs(T, B, wrap_len(T, B, L, kind) + 2, seed=14), inputs(T, B, 3, seed=15)
    a, fresh = make(route, ir), make(route, ir)
    run_stream(a, xs)
    ins = staged(xs2)
    torch.cuda.synchronize()
    sa, sb = held_stream(), torch.cuda.Stream()
    held = hold(sa)
    with torch.cuda.stream(sa):
        a.reset()
    with torch.cuda.stream(sb):
        y = launch(a, ins, form)
    pending = not held.query()
    torch.cuda.synchronize()
    assert pending, HELD
    assert same_bits(host(y), np.concatenate(run_stream(fresh, xs2)))


@pytest.mark.parametrize("form", ["process", "batch"])
def test_launch_on_a_held_stream_then_reset_on_the_default_stream(gab, make, route, form):
    """(e2) launches queued on stream B behind a hold, then reset on the default stream: the reset waits for them, so
    they give the un-reset continuation, and the buffer after the reset is a fresh plan's."""
    import torch
    T, B, L, kind = shape(route)
    ir = reverb_ir(T, L, seed=16)
    xs, xs2, x3 = inputs(T, B, wrap_len(T, B, L, kind) + 2, seed=17), inputs(T, B, 3, seed=18), inputs(T, B, 1, seed=19)
    a, twin, fresh = make(route, ir), make(route, ir), make(route, ir)
    run_stream(a, xs)
    run_stream(twin, xs)
    ins, x_next, y_next = staged(xs2), dev(x3[0]), torch.empty(T * B, device="cuda")
    torch.cuda.synchronize()
    sb = held_stream()
    held = hold(sb)
    with torch.cuda.stream(sb):
        y = launch(a, ins, form)
    a.reset()
    pending = not held.query()
    a.process(x_next, out=y_next)
    torch.cuda.synchronize()
    assert pending, HELD
    assert same_bits(host(y), np.concatenate(run_stream(twin, xs2)))
    assert same_bits(host(y_next), run_stream(fresh, x3)[0])


def test_launch_on_a_held_stream_then_set_ir_on_the_default_stream(gab, make, route):
    """(e3) a launch queued on stream B behind a hold, then set_ir(ir2) on the default stream: the launch runs with the
    taps it was queued under (the ir1 twin's bits), the launches after set_ir with the new ones (the ir2 twin's bits;
    on the split cut the first of them to rounding, see test_set_ir_mid_stream)."""
    import torch
    T, B, L, kind = shape(route)
    ir1, ir2 = reverb_ir(T, L, seed=20), reverb_ir(T, L, seed=21)
    m = fill_len(B, L) + 3
    xs = inputs(T, B, m + 3, seed=22)
    a, t1, t2 = make(route, ir1), make(route, ir1), make(route, ir2)
    run_stream(a, xs[:m])
    y1 = run_stream(t1, xs[:m + 1])[m]
    y2 = run_stream(t2, xs)[m + 1:]
    x_dev, ir2_dev, y = dev(xs[m]), dev(ir2), torch.empty(T * B, device="cuda")
    torch.cuda.synchronize()
    sb = held_stream()
    held = hold(sb)
    with torch.cuda.stream(sb):
        a.process(x_dev, out=y)
    pending = not held.query()
    a.set_ir(ir2_dev)
    after = run_stream(a, xs[m + 1:])
    torch.cuda.synchronize()
    assert pending, HELD
    assert same_bits(host(y), y1)
    peak = max(np.abs(r).max() for r in y2)
    if kind == "split":
        assert np.abs(after[0] - y2[0]).max() <= SPLIT_TOL * peak
        after, y2 = after[1:], y2[1:]
    for i, (u, v) in enumerate(zip(after, y2)):
        assert same_bits(u, v), i
