#!/usr/bin/env python3
"""Device time of one gab_xover_process beside the two things it is measured against, in the same process.
B = 512, T in {8192, 65536}, K = 2, 3, 4; white noise; splits at {1000}, {120, 2500}, {40, 400, 4000} Hz on every track.
  1. today's way of doing the same split: K EqPlan.process launches in scan form on the same input, band j's cascade
     written as biquads (second-order Butterworth low- and high-passes twice, second-order all-passes): 2 + 2,
     3 + 4 + 4 and 4 + 5 + 6 + 6 sections;
  2. gab_gain on the [T][B] block, scaled by the bytes: the plan moves 4 (1 + K) T B, gab_gain 8 T B.
Every launch is timed by its own pair of HIP events after a warm-up, the three alternated; median, p99 and largest of
`--launches` of them are reported.  process_batch(--batch, 32) is timed the same way and reported per buffer.  Two
statements per row, reported and not enforced: not slower than the EqPlan composition (the yardstick), and within 1.5 x
gab_gain's time scaled by the bytes (the aim).  The margin of both is the spread of gab_gain's own median over the rows
of one track count, printed below each group.  The last lines are the host figures of tests/test_crossover_host.py:
float32 against float64 on the four sets of splits.

    python tools/crossover_bench.py [--launches 100] [--tracks 8192,65536] [--out profiles/r20_crossover.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/crossover_bench.py --launches 50 --out /dev/null

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

FS = 48000.0
SPLITS = {2: [1000.0], 3: [120.0, 2500.0], 4: [40.0, 400.0, 4000.0]}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(t):
    return float(np.median(t)), float(np.percentile(t, 99)), float(max(t))


def band_cascades(freqs):
    """Band j of the split as scipy sections [n][6]: the biquads a user writes out today."""
    from scipy import signal
    lp = [signal.butter(2, f, "lowpass", fs=FS, output="sos") for f in freqs]
    hp = [signal.butter(2, f, "highpass", fs=FS, output="sos") for f in freqs]
    ap = [np.concatenate([s[:, 5:2:-1], s[:, 3:]], axis=1) for s in lp]          # the denominator, reversed, on top
    S = len(freqs)
    bands = []
    for j in range(S + 1):
        sec = [hp[i] for i in range(min(j, S)) for _ in (0, 1)]
        if j < S:
            sec += [lp[j], lp[j]] + [ap[m] for m in range(j + 1, S)]
        bands.append(np.concatenate(sec))
    return bands


def host_figures(emit):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_crossover_host import SETS, Twin, Twin64, noise, rows32
    for freqs in SETS:
        K, n = len(freqs) + 1, 2048
        x = noise(1, n, 20)
        twin = Twin(1, n, K)
        twin.set_splits(rows32(freqs))
        got = twin.process(x)[:, 0].astype(np.float64)
        want = Twin64(rows32(freqs)).process(x[0].astype(np.float64))
        err = np.abs(got - want).max(axis=1)
        emit("# float32 against float64, splits %s, 2048 samples of white noise: %s of the output's peak; %s of the band's own"
             % (freqs, " ".join("%.2e" % e for e in err / np.abs(want).max()),
                " ".join("%.2e" % e for e in err / np.abs(want).max(axis=1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_crossover.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/crossover_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    emit("%7s %2s | %9s %8s %8s | %8s %8s | %8s %8s | %8s %4s | %8s %6s %4s %8s | %10s %3s" % (
        "tracks", "K", "xover med", "p99", "max", "gain med", "p99", "K eq med", "p99", "of eq", "met", "aim 1.5x",
        "x gain", "met", "of 8TB/s", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        z = torch.empty_like(x)
        rows = []
        for K in (2, 3, 4):
            plan = gab.CrossoverPlan(T, B, K)
            plan.set_splits(torch.from_numpy(np.tile(gab.crossover_rows(SPLITS[K]), (T, 1, 1))).cuda())
            y = torch.empty(K * T * B, device="cuda")
            largs = plan.prepare(x, y)
            eqs = []
            for sos in band_cascades(SPLITS[K]):
                eq = gab.EqPlan(T, B, len(sos))
                eq.set_sos(sos)
                assert eq.form != (0, 0)
                eqs.append((eq, eq.prepare(x, torch.empty_like(x))))
            xs = x.repeat(NB)
            ys = torch.empty(NB * K * T * B, device="cuda")

            def run():
                plan.launch(largs)

            def gain():
                gab.gain(x, 0.5, out=z)

            def eq_way():
                for eq, eargs in eqs:
                    eq.launch(eargs)

            def batch():
                plan.process_batch(xs, out=ys)

            for _ in range(5):
                run()
                gain()
                eq_way()
            batch()
            t_p, t_g, t_e, t_b = [], [], [], []
            for _ in range(args.launches):
                t_p.append(timed(run))
                t_g.append(timed(gain))
                t_e.append(timed(eq_way))
            for _ in range(max(5, args.launches // 20)):
                t_b.append(timed(batch) / NB)
            nbytes = 4.0 * (1 + K) * T * B
            rows.append((K, stats(t_p), stats(t_g), stats(t_e), nbytes, float(np.median(t_b))))
            plan.close()
            for eq, _ in eqs:
                eq.close()
            del xs, ys, y, eqs
        gains = [r[2][0] for r in rows]
        margin = (max(gains) - min(gains)) / min(gains)
        for K, p, g, e, nbytes, tb in rows:
            scaled = g[0] * (1 + K) / 2.0
            emit("%7d %2d | %9.2f %8.2f %8.2f | %8.2f %8.2f | %8.2f %8.2f | %8.2f %4s | %8.2f %6.2f %4s %8.3f | %10.2f %3d" % (
                T, K, p[0], p[1], p[2], g[0], g[1], e[0], e[1], p[0] / e[0], "yes" if p[0] <= e[0] * (1.0 + margin) else "no",
                1.5 * scaled, p[0] / scaled, "yes" if p[0] <= 1.5 * scaled * (1.0 + margin) else "no",
                nbytes / (p[0] * 1e-6) / 8e12, tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin of `met`" % (
            T, 100.0 * margin, min(gains), max(gains)))
        del x, z
    host_figures(emit)
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
