#!/usr/bin/env python3
"""Device time of one gab_sat_process beside what a user composed before the plan existed and beside gab_gain, on the
same block, in the same process.  B = 512, T in {8192, 65536}, R = 2 and 4, the cubic curve driven 12 dB, the default
taps (32, 32 R) and (16, 16 R).  Three columns:
  (a) the yardstick   ResamplePlan (up R) -> the curve as a torch expression -> ResamplePlan (down R): the fused launch
                      must not be slower in any row, beyond the spread of gab_gain's own median over the rows of a run;
  (b) the aim         gab_gain's time on the same block: the plan moves the same 8 T B bytes.  At (Ku, Kd) the plan
                      issues R Ku + Kd fmaf a base sample (64 R at the defaults): the time at which that count would run
                      at the vector fp32 rate of the part (157.3 TFLOPS, an fmaf two of them) is printed beside it, and
                      which of the two the launch is nearer to;
  (c) gab_gain itself.
Every launch is timed by its own pair of HIP events after a warm-up, the three alternated; median, p99 and largest of
`--launches` of them are reported.  process_batch(--batch, 32) is timed the same way and reported per buffer.

    python tools/saturator_bench.py [--launches 100] [--tracks 8192,65536] [--out profiles/r29_saturator.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/saturator_bench.py --launches 50 --out /dev/null
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpuaudiobench_amd as gab  # noqa: E402

FMAF_PER_SECOND = 157.3e12 / 2.0


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
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_saturator.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/saturator_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    emit("%7s %2s %9s | %8s %8s %8s | %8s %8s | %8s %8s | %8s %4s | %8s %4s %8s %7s | %10s %3s" % (
        "tracks", "R", "taps", "sat med", "p99", "max", "gain med", "p99", "comp med", "p99", "/ comp", "met",
        "/ gain", "met", "fmaf us", "nearer", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        x = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z, w = (torch.empty_like(x) for _ in range(3))
        xs = x.repeat(NB)
        ys = torch.empty_like(xs)
        row = gab.saturator_params(drive_db=12.0, bias=0.1, level_db=-3.0)
        table = torch.from_numpy(np.tile(row, (T, 1))).cuda()
        drive, bias, level = (float(v) for v in row)
        rows = []
        for R in (2, 4):
            for Ku, Kd in ((32, 32 * R), (16, 16 * R)):
                plan = gab.SaturatorPlan(T, B, R, "cubic", Ku, Kd)
                plan.set_params(table, ramp=False)
                up, down = gab.ResamplePlan(T, B, R, 1, Ku), gab.ResamplePlan(T, R * B, 1, R, Kd)
                u = torch.empty(T * R * B, dtype=torch.float32, device="cuda")
                sargs = plan.prepare(x, y)
                sb = float(np.clip(bias, -1, 1) * (1.5 - 0.5 * np.clip(bias, -1, 1) ** 2))

                def run():
                    plan.launch(sargs)

                def gain():
                    gab.gain(x, 0.5, out=z)

                def comp():                                     # what a user wrote: two plans and a torch expression
                    up.process(x, out=u)
                    c = torch.clamp(drive * u + bias, -1.0, 1.0)
                    v = level * (c * (1.5 - 0.5 * c * c) - sb)
                    down.process(v, out=w)

                def batch():
                    plan.process_batch(xs, out=ys)

                for _ in range(5):
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
                fmaf_us = (R * Ku + Kd) * float(T) * B / FMAF_PER_SECOND * 1e6
                rows.append((R, Ku, Kd, stats(t_p), stats(t_g), stats(t_c), float(np.median(t_b)), fmaf_us))
                for p in (plan, up, down):
                    p.close()
                del u
        gains = [r[4][0] for r in rows]
        margin = (max(gains) - min(gains)) / min(gains)
        for R, Ku, Kd, p, g, c, tb, fm in rows:
            nearer = "gain" if abs(p[0] - g[0]) <= abs(p[0] - fm) else "fmaf"
            emit("%7d %2d %9s | %8.2f %8.2f %8.2f | %8.2f %8.2f | %8.2f %8.2f | %8.2f %4s | %8.2f %4s %8.2f %7s | %10.2f %3d" % (
                T, R, "%d,%d" % (Ku, Kd), p[0], p[1], p[2], g[0], g[1], c[0], c[1], p[0] / c[0],
                "yes" if p[0] <= c[0] * (1.0 + margin) else "no", p[0] / g[0],
                "yes" if p[0] <= g[0] * (1.0 + margin) else "no", fm, nearer, tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin of `met`" % (
            T, 100.0 * margin, min(gains), max(gains)))
        slower = sum(1 for r in rows if r[3][0] > r[5][0] * (1.0 + margin))
        missed = sum(1 for r in rows if r[3][0] > r[4][0] * (1.0 + margin))
        emit("# %d tracks: slower than resample + torch + resample in %d of %d rows (%.3f x to %.3f x of it); the aim "
             "(gab_gain's time) MISSED in %d of %d rows, at %.2f x to %.2f x gab_gain and %.2f x to %.2f x the fmaf time" % (
                 T, slower, len(rows), min(r[3][0] / r[5][0] for r in rows), max(r[3][0] / r[5][0] for r in rows),
                 missed, len(rows), min(r[3][0] / r[4][0] for r in rows), max(r[3][0] / r[4][0] for r in rows),
                 min(r[3][0] / r[7] for r in rows), max(r[3][0] / r[7] for r in rows)))
        del x, y, z, w, xs, ys
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
