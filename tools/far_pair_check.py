"""The split cut's batch launch (conv_split_batch12_kernel) on seeded inputs, every launch's output to one .npz:

    python tools/far_pair_check.py OUT.npz

Run once on the product library (the far role's products by bin pairs) and once on the diagnostic build with the product by own
bins (GAB_LIB_PATH=gpuaudiobench_amd/libgab_hip_ablate.so GAB_CONV_SPLIT_DEBUG=128), the two files must hold the same bits:
tests/test_far_pair_product_gpu.py.  The pairing only moves values between threads, so nothing may differ.

Cases: 4 and 8 channels (one workgroup and two), 4096 taps, 512-sample buffers; two batch launches of n buffers each,
n = 1, 2, 3 (the far groups' first windows and idle periods) and 9, 11 (windows wholly inside the launch; the second launch's
windows reach back into the ring); from a fresh plan ("even") and after one per-buffer call ("odd": head0 is odd, the two
far groups change places).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, L = 512, 4096
TS, NS, STARTS = (4, 8), (1, 2, 3, 9, 11), ("even", "odd")


def case_inputs(gab, T, n, start, launches=2):
    """The launches x n + 1 buffers of a case (the first one is used by the "odd" start alone)."""
    return [gab.harness.noise(T * B, seed=700 + 64 * T + 4 * n + k + (1000 if start == "odd" else 0)) for k in range(launches * n + 1)]


def batch_launches(gab, torch, plan, xs, n, start):
    """Batch launches of n buffers each over xs[1:] from a reset plan (two for a case's inputs) -> [len(xs) - 1][B*T]."""
    plan.reset()
    if start == "odd":
        plan.process(torch.from_numpy(xs[0]).cuda(), mode=gab.CONV_STREAMING)
    ys = [plan.process_batch(torch.from_numpy(np.concatenate(xs[1 + i * n: 1 + (i + 1) * n])).cuda(), n) for i in range((len(xs) - 1) // n)]
    return torch.cat(ys).cpu().numpy()


def routes(gab, torch):
    out = {}
    for T in TS:
        plan = gab.ConvPlan(T, B, L, scheme="split")
        plan.set_ir(torch.from_numpy(gab.harness.conv_accel_ir(L, T)).cuda())
        for n in NS:
            for start in STARTS:
                out["T%d_n%d_%s" % (T, n, start)] = batch_launches(gab, torch, plan, case_inputs(gab, T, n, start), n, start)
        plan.close()
    return out


if __name__ == "__main__":
    import torch
    import gpuaudiobench_amd as gab
    np.savez(sys.argv[1], **routes(gab, torch))
    print("far_pair_check: %s, far products %s" % (
        os.path.basename(gab._capi.LIB_PATH), "by own bins" if int(os.environ.get("GAB_CONV_SPLIT_DEBUG", "0")) & 128 else "by bin pairs"))
