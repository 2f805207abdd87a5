#!/usr/bin/env python3
"""Device time of one gab_resample_process beside two yardsticks on the same block, in the same process.  B = 512, T in
{8192, 65536}, 147 -> 160 (K = 32), 160 -> 147 (K = 40) and 1 -> 2 (K = 32):
    gain   gab_gain on the input block: 8 T B bytes, none of the work
    floor  the plan's own bytes per buffer, 4 T (B + out_capacity), at 8 TB/s
Every launch is timed by its own pair of HIP events after a warm-up; the median of `--launches` of them and the largest
are reported, the calls alternated.  process_batch(--batch, 32) is timed the same way and reported per buffer.  The
position moves from launch to launch as it does in a stream, so a median is over the whole pattern of counts.

    python tools/resample_bench.py [--launches 200] [--tracks 8192,65536]

The kernels' own times, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py --launches 50

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpuaudiobench_amd as gab  # noqa: E402

RATIOS = [(160, 147, 32), (147, 160, 40), (2, 1, 32)]      # up, down, taps: 147 -> 160, 160 -> 147, 1 -> 2


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    B, nb = 512, args.batch
    print("%7s %9s %4s | %9s %8s | %8s %8s | %8s %8s | %10s %3s | %9s" % (
        "tracks", "up/down", "taps", "resamp us", "max us", "gain us", "max us", "floor us", "of 8TB/s", "batch us/b",
        "nb", "Gfmaf/s"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y = torch.empty_like(x)
        xs = x.repeat(nb)
        for up, down, K in RATIOS:
            plan = gab.ResamplePlan(T, B, up, down, K)
            out = torch.empty(T, plan.out_capacity, dtype=torch.float32, device="cuda")
            bout = torch.empty(nb, T, plan.out_capacity, dtype=torch.float32, device="cuda")

            def resample():
                plan.process(x, out=out)

            def gain():
                gab.gain(x, 2.0, out=y)

            def batch():
                plan.process_batch(xs, out=bout)

            for _ in range(10):
                resample()
                gain()
            batch()
            t_r, t_g, t_b = [], [], []
            for _ in range(args.launches):
                t_r.append(timed(resample))
                t_g.append(timed(gain))
            for _ in range(max(5, args.launches // 20)):
                t_b.append(timed(batch) / nb)
            mr, mg, mb = (float(np.median(t)) for t in (t_r, t_g, t_b))
            nbytes = 4.0 * T * (B + plan.out_capacity)
            fmaf = float(T) * B * plan.up / plan.down * K
            print("%7d %9s %4d | %9.2f %8.2f | %8.2f %8.2f | %8.2f %8.3f | %10.2f %3d | %9.0f" % (
                T, "%d/%d" % (plan.up, plan.down), K, mr, max(t_r), mg, max(t_g), nbytes / 8e12 * 1e6,
                nbytes / (mr * 1e-6) / 8e12, mb, nb, fmaf / (mr * 1e-6) / 1e9), flush=True)
            plan.close()


if __name__ == "__main__":
    main()
