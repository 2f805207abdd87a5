"""The batch launch's far spectral products by bin pairs (conv_split_batch12_kernel: a far thread forms its eight low bins and
their partners N - k from one fetch of the spectra, the operands and the results cross in two regions of the group's LDS image):
  * two batch launches of n buffers against the same buffers through gab_conv_process one at a time, int32 view for int32 view,
    from a fresh plan and with an odd head (the two far groups change places): tools/far_pair_check.py;
  * the far share alone (taps below 1024 zero), channel a at level 1 beside channel b at 2^-10, against the float64 direct
    form within bench.py's PARITY_TOL (1e-5 of the stream's peak);
  * the product library against the diagnostic build's product by own bins (GAB_CONV_SPLIT_DEBUG=128, loaded by path in a
    child process), bit for bit: the pairing only moves values between threads."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from plan_helpers import gab  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "far_pair_check.py")
PARITY_TOL = 1e-5               # of the stream's peak: the project's tolerance (bench.py)

spec = importlib.util.spec_from_file_location("far_pair_check", TOOL)
tool = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tool)
B, L = tool.B, tool.L
CASES = [(T, n, start) for T in tool.TS for n in tool.NS for start in tool.STARTS]


def ident(c):
    return "T%d-n%d-%s" % c


@pytest.fixture(scope="module")
def product(gab):
    """The product library's batch launches, every case: computed once."""
    import torch
    assert os.path.basename(gab._capi.LIB_PATH) == "libgab_hip.so"
    return tool.routes(gab, torch)


@pytest.fixture(scope="module")
def own_bins(tmp_path_factory):
    """The same cases on the diagnostic build with every far thread forming its own sixteen bins."""
    lib = os.path.join(ROOT, "gpuaudiobench_amd", "libgab_hip_ablate.so")
    assert os.path.exists(lib), "the diagnostic library is not built (GAB_BUILD_TAG=ablate GAB_ABLATE=1 python gpuaudiobench_amd/build.py)"
    path = str(tmp_path_factory.mktemp("far_pair") / "own_bins.npz")
    r = subprocess.run([sys.executable, TOOL, path], cwd=ROOT, env=dict(os.environ, GAB_LIB_PATH=lib, GAB_CONV_SPLIT_DEBUG="128"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert "libgab_hip_ablate.so, far products by own bins" in r.stdout, r.stdout
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_the_check_covers_every_case(product, own_bins):
    assert sorted(product) == sorted("T%d_n%d_%s" % c for c in CASES) == sorted(own_bins)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_batch_launches_equal_per_buffer_calls(gab, product, case):
    import torch
    T, n, start = case
    xs = tool.case_inputs(gab, T, n, start)
    plan = gab.ConvPlan(T, B, L, scheme="split")
    plan.set_ir(torch.from_numpy(gab.harness.conv_accel_ir(L, T)).cuda())
    ys = [plan.process(torch.from_numpy(x).cuda(), mode=gab.CONV_STREAMING).cpu().numpy() for x in xs[0 if start == "odd" else 1:]]
    plan.close()
    want = np.concatenate(ys[1 if start == "odd" else 0:])
    got = product["T%d_n%d_%s" % case]
    assert got.dtype == np.float32 and got.shape == want.shape == (2 * n * T * B,)
    assert np.isfinite(got).all() and np.count_nonzero(got) > 0
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%d of %d words differ" % (
        int((got.view(np.int32) != want.view(np.int32)).sum()), got.size)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_bin_pairs_give_the_bits_of_own_bins(product, own_bins, case):
    a, b = product["T%d_n%d_%s" % case], own_bins["T%d_n%d_%s" % case]
    assert a.dtype == np.float32 and a.shape == b.shape and a.size > 0
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0.0
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "%d of %d words differ" % (
        int((a.view(np.int32) != b.view(np.int32)).sum()), a.size)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_the_far_share_alone_at_unequal_levels(gab, case):
    """Taps below 1024 zero: every output sample is the far role's.  Channel 2q at level 1, channel 2q + 1 at 2^-10.
    A stream's first two buffers have no far share (zeros), so the case's two launches are followed by two more of the
    same n: no case is all zeros."""
    import torch
    import oracle
    T, n, start = case
    ir = gab.harness.conv_accel_ir(L, T).reshape(T, L).copy()
    ir[:, :1024] = 0.0
    ir = ir.ravel()
    lv = np.where(np.arange(T) % 2 == 0, 1.0, 2.0 ** -10).astype(np.float32)
    xs = [(x.reshape(T, B) * lv[:, None]).ravel() for x in tool.case_inputs(gab, T, n, start, launches=4)]
    plan = gab.ConvPlan(T, B, L, scheme="split")
    plan.set_ir(torch.from_numpy(ir).cuda())
    got = tool.batch_launches(gab, torch, plan, xs, n, start)
    plan.close()
    hist = np.zeros(T * L, np.float32)
    refs = [oracle.conv_accel_stream(x, ir, hist, L, B, T, f64=True) for x in xs[0 if start == "odd" else 1:]]
    ref = np.concatenate(refs[1 if start == "odd" else 0:])
    peak = float(np.abs(np.concatenate(refs)).max())
    assert np.isfinite(got).all() and np.count_nonzero(got) > 0 and peak > 0
    assert np.count_nonzero(got.reshape(4 * n, B, T)[2:]) > 0.99 * (4 * n - 2) * B * T     # every buffer that has a far share
    err = float(np.abs(got - ref).max()) / peak
    print("far share T=%d n=%d %s: max error %.3e of the stream's peak %.3e" % (T, n, start, err, peak))
    assert err <= PARITY_TOL, err
