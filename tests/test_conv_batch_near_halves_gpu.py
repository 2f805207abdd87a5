"""The batch launch's near products, each divided between a pair's two near waves (conv_split_batch12_kernel: the
forward wave forms bins 0-7 per lane of the A2 share and of the A product, the pair's inverse wave bins 8-15, both
from the spectrum in the forward wave's LDS image; the forward wave hands the sum of its bins over through LDS, the
inverse wave keeps the sum of its own in registers for the next period).  What can go wrong is a hand-off: the
image read before it is written or after it is overwritten, a half taken from the other pair's image or spectra,
a half missing from the output spectrum, the first period's share (formed from the history ring's spectrum, before
any inverse transform) or the last, idle period.  Every case is held bit for bit to one
process() call per buffer on a second plan, at the smallest shapes that have these hand-offs: one duo, two and
three; taps that fill the far partition and taps that barely reach it; launches of 1, 2, 3 and 10 buffers."""
import numpy as np
import pytest

from test_conv_plan_state_gpu import bits, dev, gab, host  # noqa: F401

pytestmark = pytest.mark.gpu

B = 512
TOL = 1e-5              # against the float64 direct form, of the stream's peak (the project's gate)


def pair_of_plans(gab, T, L, ir):
    a, b = gab.ConvPlan(T, B, L, scheme="split"), gab.ConvPlan(T, B, L, scheme="split")
    assert a.scheme == "split" and b.scheme == "split"
    a.set_ir(dev(ir))
    b.set_ir(dev(ir))
    return a, b


def per_buffer(plan, xs):
    return [host(plan.process(dev(x))) for x in xs]


def batch(plan, xs):
    n, size = len(xs), xs[0].size
    return list(host(plan.process_batch(dev(np.concatenate(xs)), n)).reshape(n, size))


def walk(a, b, xs, n, lead):
    """`lead` single launches, a batch of n, one single launch, a batch of n on `b`; one launch per buffer on `a`."""
    assert len(xs) == lead + 2 * n + 1
    want = per_buffer(a, xs)
    got = per_buffer(b, xs[:lead]) + batch(b, xs[lead:lead + n]) + per_buffer(b, xs[lead + n:lead + n + 1]) + batch(b, xs[lead + n + 1:])
    for k, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(bits(w), bits(g)), "buffer %d of %d (lead %d, n %d)" % (k, len(xs), lead, n)
    assert b.scheme == "split"
    return got


@pytest.mark.parametrize("n", [1, 2, 3, 10])
@pytest.mark.parametrize("L", [4096, 1100])
@pytest.mark.parametrize("T", [4, 8, 12])
def test_batches_equal_one_launch_per_buffer(gab, orc, T, L, n):
    """Two batches of n with a single launch between them start at history heads 0 and n + 1; after reset() the same
    behind one leading single launch start at heads 1 and n + 2: every n meets both parities of the head, so both far
    groups start first, and n = 1, 2 are launches that are little more than the first period's share and the last,
    idle period."""
    a, b = pair_of_plans(gab, T, L, orc.conv_accel_ir(L, T))
    try:
        walk(a, b, [orc.noise(T * B, seed=700 + i) for i in range(2 * n + 1)], n, 0)
        a.reset()
        b.reset()
        walk(a, b, [orc.noise(T * B, seed=800 + i) for i in range(2 * n + 2)], n, 1)
    finally:
        a.close()
        b.close()


def test_a_silent_channel_and_a_silent_pair_keep_to_their_pairs(gab, orc):
    """Two duos.  Pair 0: channel 0 silent beside a loud partner; pair 1 (the same workgroup's other pair): all zeros;
    pair 2 loud; pair 3: channel 7 silent beside a partner 2^10 louder than the rest.  A half taken from the other pair's
    image or spectra breaks the equality with the per-buffer launches, and puts something into the silent pair."""
    T, L, n = 8, 4096, 3
    gain = np.array([0, 1, 0, 0, 1, 1, 2.0 ** 10, 0], np.float32)
    xs = [(orc.noise(T * B, seed=900 + i).reshape(T, B) * gain[:, None]).ravel() for i in range(2 * n + 1)]
    a, b = pair_of_plans(gab, T, L, orc.conv_accel_ir(L, T))
    try:
        got = np.stack(walk(a, b, xs, n, 0)).reshape(len(xs), B, T)             # outputs are sample-major: [B][T]
    finally:
        a.close()
        b.close()
    assert not got[:, :, 2:4].any()                                            # the silent pair: zeros, either sign
    assert got[:, :, 1].any() and got[:, :, 4].any() and got[:, :, 5].any() and got[:, :, 6].any()


def test_a_batch_is_the_float64_direct_form(gab, orc):
    """Ten buffers in one launch (the far partition's window fills at the eighth) against the oracle's float64
    direct form, 1e-5 of the stream's peak."""
    T, L, n = 4, 4096, 10
    ir = orc.conv_accel_ir(L, T)
    xs = [orc.noise(T * B, seed=42 + i) for i in range(n)]
    p = gab.ConvPlan(T, B, L, scheme="split")
    try:
        assert p.scheme == "split"
        p.set_ir(dev(ir))
        ys = batch(p, xs)
    finally:
        p.close()
    hist = np.zeros(T * L, np.float32)
    err, peak = 0.0, 0.0
    for x, y in zip(xs, ys):
        ref = orc.conv_accel_stream(x, ir, hist, L, B, T, f64=True)
        err = max(err, float(np.abs(y - ref).max()))
        peak = max(peak, float(np.abs(ref).max()))
    print("\nbatch of %d against the float64 direct form: %.3g of peak" % (n, err / peak))
    assert peak > 0 and err / peak <= TOL, err / peak
