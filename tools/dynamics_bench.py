#!/usr/bin/env python3
"""Device time of one gab_dyn_process beside gab_gain and a one-section gab_eq_process on the same block, in the same
process.  B = 512, T in {8192, 65536}; hard and soft knee, with and without a key block, link 1 and 2.  The tracks
compress: noise 12 dB over a threshold at ratio 4, attack 5 ms, release 100 ms.
Every launch is timed by its own pair of HIP events after a warm-up, the three calls alternated; median, p99 and
largest of `--launches` of them are reported.  process_batch(--batch, 32) is timed the same way and reported per
buffer.  The plan moves 8 T B bytes per buffer (x in, y out), 12 T B with a key; gab_gain moves 8 T B.  The aim is
1.5 x gab_gain's median from the same row, scaled by 12 / 8 with a key; it is reported, not enforced.

    python tools/dynamics_bench.py [--launches 200] [--tracks 8192,65536] [--out profiles/r14_dynamics.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/dynamics_bench.py --launches 50 --out /dev/null

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpuaudiobench_amd as gab  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(t):
    return float(np.median(t)), float(np.percentile(t, 99)), float(max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_dynamics.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/dynamics_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    emit("%7s %5s %4s %4s | %8s %8s %8s | %8s %8s %8s | %8s %8s %8s | %8s %4s %8s | %10s %3s" % (
        "tracks", "knee", "key", "link", "dyn med", "p99", "max", "gain med", "p99", "max", "eq1 med", "p99", "max",
        "aim", "met", "of 8TB/s", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        x = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        k = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z, w = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        xs, ks = x.repeat(NB), k.repeat(NB)
        ys = torch.empty_like(xs)
        eq = gab.EqPlan(T, B, 1)
        eargs = eq.prepare(x, w)
        for knee_db in (0.0, 6.0):
            for keyed in (False, True):
                for link in (1, 2):
                    plan = gab.DynamicsPlan(T, B, link)
                    # uniform noise in [-1, 1] has an RMS of -4.8 dB: most samples sit around 12 dB over -18 dB
                    row = gab.dynamics_params(-18.0, 4.0, knee_db, 5.0, 100.0, makeup_db=3.0)
                    plan.set_params(torch.from_numpy(np.tile(row, (T, 1))).cuda(), ramp=False)
                    largs = plan.prepare(x, y, key=k if keyed else None)

                    def run():
                        plan.launch(largs)

                    def gain():
                        gab.gain(x, 0.5, out=z)

                    def eq1():
                        eq.launch(eargs)

                    def batch():
                        plan.process_batch(xs, key=ks if keyed else None, out=ys)

                    for _ in range(10):
                        run()
                        gain()
                        eq1()
                    batch()
                    t_d, t_g, t_e, t_b = [], [], [], []
                    for _ in range(args.launches):
                        t_d.append(timed(run))
                        t_g.append(timed(gain))
                        t_e.append(timed(eq1))
                    for _ in range(max(5, args.launches // 20)):
                        t_b.append(timed(batch) / NB)
                    d, g, e = stats(t_d), stats(t_g), stats(t_e)
                    nbytes = (12.0 if keyed else 8.0) * T * B
                    aim = 1.5 * g[0] * nbytes / (8.0 * T * B)
                    emit("%7d %5s %4s %4d | %8.2f %8.2f %8.2f | %8.2f %8.2f %8.2f | %8.2f %8.2f %8.2f | %8.2f %4s %8.3f | %10.2f %3d" % (
                        T, "soft" if knee_db else "hard", "yes" if keyed else "no", link, d[0], d[1], d[2], g[0], g[1],
                        g[2], e[0], e[1], e[2], aim, "yes" if d[0] <= aim else "no", nbytes / (d[0] * 1e-6) / 8e12,
                        float(np.median(t_b)), NB))
                    plan.close()
        eq.close()
        del x, k, y, z, w, xs, ks, ys
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
