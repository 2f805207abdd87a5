#!/usr/bin/env python3
"""Device time of one gab_lim_process beside gab_gain and beside what the headers recommended for look-ahead before the
plan existed, gab_delay_process followed by gab_dyn_process with the undelayed block as its key (two launches), on the
same block, in the same process.  B = 512, T in {8192, 65536}, W = 64 and 256 (k = 6 and 8), full-scale noise under a
ceiling that is hit all the time (-12 dB) and one that never is (+12 dB), release 100 ms; link 1, and under the ceiling
that is hit also link 64 (every 64 tracks on one detector, in the limiter and in the compressor of the composition): the
limiter then takes two launches a buffer, the detector's in front, and its batch goes buffer by buffer.
Every launch is timed by its own pair of HIP events after a warm-up, the three alternated; median, p99 and largest of
`--launches` of them are reported.  process_batch(--batch, 32) is timed the same way and reported per buffer.  The plan
moves 8 T B bytes per buffer (x in, y out), as gab_gain does.  Two yardsticks, reported and not enforced: the
composition's median from the same row (the plan should not be slower), and 1.5 x gab_gain's median from the same row.
The margin of both is the spread of gab_gain's own median over the rows of one track count, printed below each group.

    python tools/limiter_bench.py [--launches 200] [--tracks 8192,65536] [--out profiles/r21_limiter.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/limiter_bench.py --launches 50 --out /dev/null

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_limiter.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/limiter_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    emit("%7s %4s %4s %4s | %8s %8s %8s | %8s %8s | %8s %8s | %8s %4s | %8s %4s %8s | %10s %3s" % (
        "tracks", "W", "hit", "link", "lim med", "p99", "max", "gain med", "p99", "comp med", "p99", "/ comp", "met",
        "aim", "met", "of 8TB/s", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        x = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z, d, w = (torch.empty_like(x) for _ in range(4))
        xs = x.repeat(NB)
        ys = torch.empty_like(xs)
        rows = []
        for W in (64, 256):
            for hit, link in ((False, 1), (True, 1), (True, 64)):
                ceil_db = -12.0 if hit else 12.0
                plan = gab.LimiterPlan(T, B, W, link)
                plan.set_params(torch.from_numpy(np.tile(gab.limiter_params(ceil_db, 100.0), (T, 1))).cuda(), ramp=False)
                delay = gab.DelayPlan(T, B, W)
                delay.set_params(torch.from_numpy(np.tile(np.array([W - 1, 0, 1, 0], np.float32), (T, 1))).cuda(), ramp=False)
                dyn = gab.DynamicsPlan(T, B, link)
                dyn.set_params(torch.from_numpy(np.tile(gab.dynamics_params(ceil_db, np.inf, 0.0, 0.0, 100.0),
                                                        (T, 1))).cuda(), ramp=False)
                largs, dargs, cargs = plan.prepare(x, y), delay.prepare(x, d), dyn.prepare(d, w, key=x)

                def run():
                    plan.launch(largs)

                def gain():
                    gab.gain(x, 0.5, out=z)

                def comp():
                    delay.launch(dargs)
                    dyn.launch(cargs)

                def batch():
                    plan.process_batch(xs, out=ys)

                for _ in range(10):
                    run()
                    gain()
                    comp()
                batch()
                t_p, t_g, t_c, t_b = [], [], [], []
                for _ in range(args.launches):
                    t_p.append(timed(run))
                    t_g.append(timed(gain))
                    t_c.append(timed(comp))
                for _ in range(max(5, args.launches // 20)):
                    t_b.append(timed(batch) / NB)
                rows.append((W, hit, link, stats(t_p), stats(t_g), stats(t_c), float(np.median(t_b))))
                for p in (plan, delay, dyn):
                    p.close()
        gains = [r[4][0] for r in rows]
        margin = (max(gains) - min(gains)) / min(gains)
        for W, hit, link, p, g, c, tb in rows:
            aim = 1.5 * g[0]
            emit("%7d %4d %4s %4d | %8.2f %8.2f %8.2f | %8.2f %8.2f | %8.2f %8.2f | %8.2f %4s | %8.2f %4s %8.3f | %10.2f %3d" % (
                T, W, "yes" if hit else "no", link, p[0], p[1], p[2], g[0], g[1], c[0], c[1], p[0] / c[0],
                "yes" if p[0] <= c[0] * (1.0 + margin) else "no", aim, "yes" if p[0] <= aim * (1.0 + margin) else "no",
                8.0 * T * B / (p[0] * 1e-6) / 8e12, tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin of `met`" % (
            T, 100.0 * margin, min(gains), max(gains)))
        slower = sum(1 for r in rows if r[3][0] > r[5][0] * (1.0 + margin))
        missed = sum(1 for r in rows if r[3][0] > 1.5 * r[4][0] * (1.0 + margin))
        emit("# %d tracks: slower than delay + dynamics in %d of %d rows (%.2f x to %.2f x of it); the aim (1.5 x gab_gain) "
             "MISSED in %d of %d rows, at %.2f x to %.2f x gab_gain" % (
                 T, slower, len(rows), min(r[3][0] / r[5][0] for r in rows), max(r[3][0] / r[5][0] for r in rows),
                 missed, len(rows), min(r[3][0] / r[4][0] for r in rows), max(r[3][0] / r[4][0] for r in rows)))
        del x, y, z, d, w, xs, ys
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
