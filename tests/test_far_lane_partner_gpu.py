"""The batch launch's far partner trade by lane-half swaps (conv_split_batch12_kernel: the far threads are renamed so that the
holder of a thread's partner bins is lane ^ 32 of its wave; threads 0 and 128 are their own partners), on inputs that load
the self-partner lanes: DC (bin 0), the alternating +-1 sequence (bin 2048), tones exactly on bins 256 r (thread 0) and
128 + 256 r (thread 128), seeded noise — one kind per channel, the two channels of a pair at levels 1 and 2^-10.
  * batch launches of n buffers, twice in a row, from a fresh plan and after one per-buffer call (odd head0), against one
    gab_conv_process launch per buffer (conv_split_kernel, which has no trade), int32 view for int32 view;
  * the same output against the float64 direct form within the project's 1e-5 of the stream's peak."""
import functools

import numpy as np
import pytest

from plan_helpers import gab  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

B, L = 512, 4096
PARITY_TOL = 1e-5               # of the stream's peak: the project's tolerance (bench.py)
CASES = [(T, n, start) for T in (4, 8) for n in (2, 3, 11) for start in ("even", "odd")]


def ident(c):
    return "T%d-n%d-%s" % c


def stream(T, count, seed):
    """[count][T * B] buffers, channel-major, of a continuous stream: channel c carries kind (c + c // 4) % 4 at level 1
    (even c) or 2^-10 (odd c)."""
    rng = np.random.default_rng(seed)
    n = np.arange(count * B, dtype=np.float64)
    tones = np.zeros_like(n)
    for r in range(8):
        if r:
            tones += np.cos(2 * np.pi * (256 * r) * n / 4096 + rng.uniform(0, 2 * np.pi))
        tones += np.cos(2 * np.pi * (128 + 256 * r) * n / 4096 + rng.uniform(0, 2 * np.pi))
    kinds = [np.ones_like(n), 1.0 - 2.0 * (n % 2), tones / 15.0, rng.uniform(-1.0, 1.0, n.size)]
    x = np.empty((T, count * B), np.float32)
    for c in range(T):
        x[c] = kinds[(c + c // 4) % 4] * (1.0 if c % 2 == 0 else 2.0 ** -10)
    return [np.ascontiguousarray(x[:, k * B:(k + 1) * B]).ravel() for k in range(count)]


@functools.lru_cache(maxsize=None)
def run(case):
    """(batch launches, per-buffer launches, float64 direct form, that form's peak over the whole stream) of a case."""
    import torch
    import oracle
    import gpuaudiobench_amd as g
    T, n, start = case
    odd = start == "odd"
    xs = stream(T, 2 * n + 1, seed=3000 + 64 * T + 4 * n + odd)
    if not odd:
        xs = xs[1:]
    ir = g.harness.conv_accel_ir(L, T)
    plan = g.ConvPlan(T, B, L, scheme="split")
    plan.set_ir(torch.from_numpy(ir).cuda())
    if odd:
        plan.process(torch.from_numpy(xs[0]).cuda(), mode=g.CONV_STREAMING)
    lo = 1 if odd else 0
    got = torch.cat([plan.process_batch(torch.from_numpy(np.concatenate(xs[lo + i * n: lo + (i + 1) * n])).cuda(), n)
                     for i in range(2)]).cpu().numpy()
    plan.reset()
    want = np.concatenate([plan.process(torch.from_numpy(x).cuda(), mode=g.CONV_STREAMING).cpu().numpy() for x in xs][lo:])
    plan.close()
    hist = np.zeros(T * L, np.float32)
    refs = [oracle.conv_accel_stream(x, ir, hist, L, B, T, f64=True) for x in xs]
    return got, want, np.concatenate(refs[lo:]), float(np.abs(np.concatenate(refs)).max())


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_batch_launches_equal_per_buffer_launches(gab, case):
    T, n, _ = case
    got, want, _, _ = run(case)
    assert got.dtype == np.float32 and got.shape == want.shape == (2 * n * T * B,)
    assert np.isfinite(got).all() and np.count_nonzero(got) > 0
    for c in range(T):                                                # every channel of every case is non-silent
        assert np.count_nonzero(got.reshape(2 * n, B, T)[:, :, c]) > 0, c
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%d of %d words differ" % (
        int((got.view(np.int32) != want.view(np.int32)).sum()), got.size)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_within_the_projects_tolerance_of_the_float64_direct_form(gab, case):
    got, _, ref, peak = run(case)
    assert np.isfinite(got).all() and np.count_nonzero(got) > 0 and peak > 0
    err = float(np.abs(got - ref).max()) / peak
    print("far lane partners T=%d n=%d %s: max error %.3e of the stream's peak %.3e" % (case + (err, peak)))
    assert err <= PARITY_TOL, err
