#!/usr/bin/env python3
"""Device time of one gab_delay_process beside gab_gain on the same block, in the same process.  B = 512, T in
{8192, 65536}, both interpolations, four settings:
    a  delay >= B, feedback 0        b  delay >= B, feedback 0.5
    c  delay 100, feedback 0.5       d  delay = min_delay, feedback 0.5 (a dependent chain of B steps per track)
Every launch is timed by its own pair of HIP events after a warm-up; the median of `--launches` of them and the largest
are reported, the two calls alternated.  process_batch(--batch, 32) is timed the same way and reported per buffer, its
length in the last column.  Beside the times: the plan's own bytes per buffer, 16 T B (x in, y out, line in, line out),
as a fraction of 8 TB/s, and the aim for a and b: twice gain's time plus a quarter.

    python tools/delay_bench.py [--launches 200] [--tracks 8192,65536]

The kernels' own times, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/delay_bench.py --launches 50

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
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
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    B, NB = 512, args.batch
    print("%7s %9s %7s | %8s %8s | %8s %8s | %8s %6s | %8s | %9s %3s" % (
        "tracks", "interp", "setting", "delay us", "max us", "gain us", "max us", "aim us", "met", "of 8TB/s", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z = torch.empty_like(x), torch.empty_like(x)
        nb = NB
        xs = x.repeat(nb)
        ys = torch.empty_like(xs)
        for interp in ("linear", "lagrange3"):
            lo = 2 if interp == "lagrange3" else 1
            for name, delay, fb in (("a", 600.5, 0.0), ("b", 600.5, 0.5), ("c", 100.0, 0.5), ("d", float(lo), 0.5)):
                plan = gab.DelayPlan(T, B, 1024, interp)
                p = np.zeros((T, 4), np.float32)
                p[:] = (delay, fb, 0.5, 0.5)
                plan.set_params(torch.from_numpy(p).cuda(), ramp=False)
                largs = plan.prepare(x, y)

                def run():
                    plan.launch(largs)

                def gain():
                    gab.gain(x, 0.5, out=z)

                def batch():
                    plan.process_batch(xs, out=ys)

                for _ in range(10):
                    run()
                    gain()
                batch()
                t_d, t_g, t_b = [], [], []
                for _ in range(args.launches):
                    t_d.append(timed(run))
                    t_g.append(timed(gain))
                for _ in range(max(5, args.launches // 20)):
                    t_b.append(timed(batch) / nb)
                md, mg, mb = float(np.median(t_d)), float(np.median(t_g)), float(np.median(t_b))
                aim = 2.25 * mg
                print("%7d %9s %7s | %8.2f %8.2f | %8.2f %8.2f | %8.2f %6s | %8.3f | %9.2f %3d" % (
                    T, interp, name, md, max(t_d), mg, max(t_g), aim,
                    ("yes" if md <= aim else "no") if name in "ab" else "-", 16.0 * T * B / (md * 1e-6) / 8e12, mb, nb),
                    flush=True)
                plan.close()


if __name__ == "__main__":
    main()
