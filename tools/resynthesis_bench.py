#!/usr/bin/env python3
"""Device time of one gab_resyn_process beside gab_gain and beside the composition a user needed before the plan
existed, on the same rows, in the same process: torch.fft.irfft of the rows, a window multiply, an add of every frame
into a carried tail, and a slice, with the tail carried by a torch copy.
B = 512, T in {8192, 65536}, H in {512, 256}.  Every call is timed by its own pair of HIP events after a warm-up, the
three alternated; medians of `--launches` of them are reported.  process_batch(--batch, 32) is timed the same way and
reported per buffer.

Two yardsticks, reported and not enforced:
  * the composition's median from the same row: the plan should not be slower;
  * the aim: the call's own bytes (rows in, block out, the accumulator read and written) at the rate gab_gain reaches on
    its bytes (block in, block out), as the ratio of the two rates.
Each reads met, missed, or "margin": inside the margin, which is how much gab_gain's own median moved between the rows of
one track count.

In front of the timings: the accuracy ratio of tests/test_resynthesis_gpu.py, the kernel's largest
max_n |u - u64| / (peak_t + peak_p) over the twin's (tests/resynthesis_twin.py) on the same rows.

    python tools/resynthesis_bench.py [--launches 200] [--tracks 8192,65536] [--out profiles/r26_resynthesis.txt]

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpuaudiobench_amd as gab  # noqa: E402
from spectrum_bench import timed, verdict  # noqa: E402

N, BINS = 1024, 513


def accuracy(emit):
    import conv_pair_twin as tw
    import resynthesis_twin as rt
    emit("# accuracy, H = B = 1024 under an all-ones window (a call's output is the previous frame's u), 4 frames of")
    emit("# noise rows at conv_pair_twin.levels(T), seed 200 + T:")
    emit("# c = max over tracks and frames of max_n |u - u64| / (peak_t + peak_p), the peaks in time")
    worst = 0.0
    for T in (1, 2, 3, 9, 17):
        rows = rt.noise_rows(4, T, seed=200 + T)
        u64 = rt.truth(rows)
        c_twin = tw.c_max(rt.figures(rt.frames_f32(rows), u64)[0])
        plan = gab.ResynthesisPlan(T, 1024, 1024)
        plan.set_window(torch.ones(N, device="cuda"))
        fed = np.concatenate([rows, np.zeros((1, T, BINS, 2), np.float32)])
        u = plan.process_batch(torch.from_numpy(fed).cuda(), 5).cpu().numpy()[1:]
        plan.close()
        c_gpu = tw.c_max(rt.figures(u, u64)[0])
        worst = max(worst, c_gpu / c_twin)
        emit("#   T %2d  c_twin %.3g  c_gpu %.3g  ratio %.2f" % (T, c_twin, c_gpu, c_gpu / c_twin))
    emit("# largest ratio %.2f: %s the factor 4 of tests/test_fft_levels_gpu.py" % (
        worst, "inside" if worst <= 4.0 else "ABOVE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_resynthesis.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/resynthesis_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    accuracy(emit)
    emit("%7s %4s | %9s %8s %8s | %7s %6s | %10s %9s %6s | %10s %3s" % (
        "tracks", "H", "resyn med", "gain med", "comp med", "/ comp", "", "resyn GB/s", "gain GB/s", "aim",
        "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        x = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        z = torch.empty_like(x)
        frame = torch.from_numpy(rng.uniform(-1, 1, T * BINS * 2).astype(np.float32)).cuda().view(1, T, BINS, 2)
        table = []
        for H in (512, 256):
            per = B // H
            plan = gab.ResynthesisPlan(T, B, H)
            g = plan.state()[1]
            rows = frame.repeat(per, 1, 1, 1).contiguous()
            rows_b = frame.repeat(per * NB, 1, 1, 1).contiguous()
            out = torch.empty((T, B), device="cuda")
            outs = torch.empty((NB, T, B), device="cuda")
            pargs = plan.prepare(rows, out)
            tail = torch.zeros(T, N, device="cuda")
            y = torch.empty((T, B), device="cuda")
            pad = torch.zeros(T, B, device="cuda")

            def run():
                plan.launch(pargs)

            def gain():
                gab.gain(x, 0.5, out=z)

            def comp():
                fr = torch.fft.irfft(torch.view_as_complex(rows), n=N, dim=-1) * g         # [per, T, 1024]
                buf = torch.cat([tail, pad], dim=1)                                     # column i: y[p - N + i]
                for j in range(per):
                    buf[:, (j + 1) * H:(j + 1) * H + N] += fr[j]
                y.copy_(buf[:, :B])
                tail.copy_(buf[:, B:])

            def batch():
                plan.process_batch(rows_b, NB, out=outs)

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
            own = 4.0 * rows.numel() + 4.0 * T * B + 2 * 4.0 * T * N
            table.append((H, float(np.median(t_p)), float(np.median(t_g)), float(np.median(t_c)),
                          float(np.median(t_b)), own))
            plan.close()
            del rows, rows_b, out, outs, tail, y, pad
        gains = [r[2] for r in table]
        margin = (max(gains) - min(gains)) / min(gains)
        for H, p, gn, c, tb, own in table:
            r_plan, r_gain = own / (p * 1e-6) / 1e9, 8.0 * T * B / (gn * 1e-6) / 1e9
            emit("%7d %4d | %9.2f %8.2f %8.2f | %7.2f %6s | %10.0f %9.0f %6s | %10.2f %3d" % (
                T, H, p, gn, c, p / c, verdict(p, c, margin), r_plan, r_gain,
                verdict(r_plan, r_gain, margin, lower_is_better=False), tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin" % (
            T, 100.0 * margin, min(gains), max(gains)))
        del x, z, frame
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
