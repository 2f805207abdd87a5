#!/usr/bin/env python3
"""Device time of one gab_mix_process beside what a user of the library had to do before it: torch.matmul on the same
float32 operands ([M x T] gains, [T x B] samples).  T in {1024, 8192, 65536}, B = 512, M in {2, 16, 64}, both input
layouts, steady buffers and ramp buffers.  Steady: HIP events around `--launches` launches of each after a warm-up, the
two alternated in the same process.  Ramp: every buffer needs its own set_gains (synchronous), so each launch is timed
by its own pair of events and the median is reported; it includes the copy that makes current := target.  Beside the
times: the plan's own bytes 4 (T B + M B + T M) (+ 4 T M on a ramp buffer) and the fraction of 8 TB/s they come to.
The library call is given the layout it likes best: for sample-major input its operand is the [B x T] buffer as it
lies (out[B x M] = X^T G), so neither side pays for a transpose.

    python tools/mix_bench.py [--launches 200] [--tracks 1024,8192,65536] [--buses 2,16,64]

The kernels' own times, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/mix_bench.py --launches 50

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpuaudiobench_amd as gab  # noqa: E402


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="1024,8192,65536")
    ap.add_argument("--buses", default="2,16,64")
    args = ap.parse_args()
    B = 512
    print("%7s %3s %7s %6s %6s | %9s %9s %6s | %9s %8s" % ("tracks", "M", "layout", "buffer", "form", "mix us", "matmul us",
                                                          "ratio", "mix bytes", "of 8TB/s"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        for M in [int(v) for v in args.buses.split(",")]:
            g = [torch.from_numpy(np.random.RandomState(2 + k).uniform(-1, 1, (T, M)).astype(np.float32)).cuda() for k in range(2)]
            gt = g[0].t().contiguous()                                   # [M][T]
            y = torch.empty(M * B, dtype=torch.float32, device="cuda")
            for layout in ("track", "sample"):
                plan = gab.MixPlan(T, B, M)
                plan.set_gains(g[0], ramp=False)
                mix_args = plan.prepare(x, y, layout=layout)
                if layout == "track":
                    xm, z = x.view(T, B), torch.empty(M, B, dtype=torch.float32, device="cuda")

                    def gemm():
                        torch.matmul(gt, xm, out=z)
                else:
                    xm, z = x.view(B, T), torch.empty(B, M, dtype=torch.float32, device="cuda")

                    def gemm():
                        torch.matmul(xm, g[0], out=z)

                def mix():
                    plan.launch(mix_args)

                for _ in range(20):
                    mix()
                    gemm()
                t_mix, t_gemm = [], []
                rounds = 4
                for _ in range(rounds):                                  # alternated: both see the same clocks
                    t_mix.append(events(mix, max(1, args.launches // rounds)))
                    t_gemm.append(events(gemm, max(1, args.launches // rounds)))
                t_mix, t_gemm = float(np.median(t_mix)), float(np.median(t_gemm))
                L, G = plan.form
                nbytes = 4 * (T * B + M * B + T * M)

                def row(kind, t, nb):
                    print("%7d %3d %7s %6s %6s | %9.2f %9.2f %6.2f | %9.3g %8.3f"
                          % (T, M, layout, kind, "%dx%d" % (L, G), t, t_gemm, t_gemm / t, nb, nb / (t * 1e-6) / 8e12), flush=True)

                row("steady", t_mix, nbytes)
                t_ramp = []
                for k in range(max(8, args.launches // 8)):
                    plan.set_gains(g[(k + 1) & 1])                       # a ramp to the other matrix
                    t_ramp.append(events(mix, 1))
                row("ramp", float(np.median(t_ramp)), nbytes + 4 * T * M)
                plan.close()


if __name__ == "__main__":
    main()
