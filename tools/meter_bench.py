#!/usr/bin/env python3
"""Device time of one gab_meter_process beside three yardsticks on the same block, in the same process.  B = 512, T in
{8192, 65536}, window in {1, 38}:
    gainstats  gab_gainstats on the block: twice the bytes (it writes a scaled copy), none of the work
    eq2        an EqPlan of two sections on the block: the K filter's work, and a block written as well
    floor      the plan's own bytes per buffer, 4 T (B + 8 + window + 1), at 8 TB/s
Every launch is timed by its own pair of HIP events after a warm-up; the median of `--launches` of them and the largest
are reported, the calls alternated.  process_batch(--batch, 32) is timed the same way and reported per buffer.

    python tools/meter_bench.py [--launches 200] [--tracks 8192,65536] [--windows 1,38]

The kernels' own times, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/meter_bench.py --launches 50

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpuaudiobench_amd as gab  # noqa: E402


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
    ap.add_argument("--windows", default="1,38")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    B, nb = 512, args.batch
    print("%7s %6s | %8s %8s | %9s %8s | %8s %8s | %8s %8s | %10s %3s" % (
        "tracks", "window", "meter us", "max us", "gainst us", "max us", "eq2 us", "max us", "floor us", "of 8TB/s",
        "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y = torch.empty_like(x)
        stats = torch.empty(2 * T, dtype=torch.float32, device="cuda")
        xs = x.repeat(nb)
        eq = gab.EqPlan(T, B, 2)
        k = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]], np.float32)
        eq.set_coeffs(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(k, (T, 2, 5)))).cuda())
        eargs = eq.prepare(x, y)
        gargs = (eargs[1], eargs[2], C.c_void_p(stats.data_ptr()), T, B, 0.5, eargs[3])
        for W in [int(v) for v in args.windows.split(",")]:
            plan = gab.MeterPlan(T, B, W)
            rows = torch.empty(T, 8, dtype=torch.float32, device="cuda")
            brows = torch.empty(nb, T, 8, dtype=torch.float32, device="cuda")
            margs = plan.prepare(x, rows)

            def meter():
                plan.launch(margs)

            def gainstats():
                gab.check(gab.lib.gab_gainstats(*gargs))

            def eq2():
                eq.launch(eargs)

            def batch():
                plan.process_batch(xs, out=brows)

            for _ in range(10):
                meter()
                gainstats()
                eq2()
            batch()
            t_m, t_g, t_e, t_b = [], [], [], []
            for _ in range(args.launches):
                t_m.append(timed(meter))
                t_g.append(timed(gainstats))
                t_e.append(timed(eq2))
            for _ in range(max(5, args.launches // 20)):
                t_b.append(timed(batch) / nb)
            mm, mg, me, mb = (float(np.median(t)) for t in (t_m, t_g, t_e, t_b))
            nbytes = 4.0 * T * (B + 8 + W + 1)
            print("%7d %6d | %8.2f %8.2f | %9.2f %8.2f | %8.2f %8.2f | %8.2f %8.3f | %10.2f %3d" % (
                T, W, mm, max(t_m), mg, max(t_g), me, max(t_e), nbytes / 8e12 * 1e6, nbytes / (mm * 1e-6) / 8e12, mb, nb),
                flush=True)
            plan.close()
        eq.close()


if __name__ == "__main__":
    main()
