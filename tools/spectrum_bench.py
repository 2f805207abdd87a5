#!/usr/bin/env python3
"""Device time of one gab_spec_process beside gab_gain and beside the composition a user needed before the plan
existed, on the same block, in the same process: a torch concatenation of the carried tail and the block, a window
multiply, gab_fft_r2c_1024, and (power rows) a torch square and scale, with the tail carried by a torch copy.  The
composition never sums bands: beside a band row stands the composition's bin form, which does less.
B = 512, T in {8192, 65536}, H in {512, 256}, modes complex, bins (power per bin) and 31 bands (logarithmic edges).
Every call is timed by its own pair of HIP events after a warm-up, the three alternated; medians of `--launches` of
them are reported.  process_batch(--batch, 32) is timed the same way and reported per buffer.

Two yardsticks, reported and not enforced:
  * the composition's median from the same row: the plan should not be slower;
  * the aim: the call's own bytes (block in, rows out) at the rate gab_gain reaches on its bytes (block in, block out),
    as the ratio of the two rates.
Each reads met, missed, or "margin": inside the margin, which is how much gab_gain's own median moved between the rows of
one track count.

In front of the timings: the accuracy ratio of tests/test_spectrum_gpu.py, the kernel's largest
max_k |X - X64| / (peak_t + peak_p) over the twin's (tests/spectrum_twin.py) on the same Hann frames.

    python tools/spectrum_bench.py [--launches 200] [--tracks 8192,65536] [--out profiles/r22_spectrum.txt]

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

N, BINS = 1024, 513


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def verdict(value, against, margin, lower_is_better=True):
    """met / missed / margin: `value` against `against`, within the relative margin."""
    if abs(value - against) <= margin * against:
        return "margin"
    return "met" if (value < against) == lower_is_better else "missed"


def accuracy(emit):
    import conv_pair_twin as tw
    import spectrum_twin as st
    emit("# accuracy, complex rows, Hann, B = H = 512, 4096 samples of noise at conv_pair_twin.levels(T), seed 100 + T:")
    emit("# c = max over tracks and frames of max_k |X - X64| / (peak_t + peak_p)")
    worst = 0.0
    for T in (1, 2, 3, 9, 17):
        x = st.noise(T, 4096, seed=100 + T)
        frames = st.windowed(x, st.frame_ends(0, 4096, 512), st.window_hann())
        X64 = st.truth(frames)
        c_twin = tw.c_max(st.figures(st.spectra(frames), X64)[0])
        plan = gab.SpectrumPlan(T, 512, 512, "complex")
        rows = torch.cat([plan.process(torch.from_numpy(b).cuda()).clone() for b in st.blocks(x, 512)]).cpu().numpy()
        plan.close()
        rows = rows.astype(np.float64)
        c_gpu = tw.c_max(st.figures(rows[..., 0] + 1j * rows[..., 1], X64)[0])
        worst = max(worst, c_gpu / c_twin)
        emit("#   T %2d  c_twin %.3g  c_gpu %.3g  ratio %.2f" % (T, c_twin, c_gpu, c_gpu / c_twin))
    emit("# largest ratio %.2f: %s the factor 4 of tests/test_fft_levels_gpu.py" % (
        worst, "inside" if worst <= 4.0 else "ABOVE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_spectrum.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/spectrum_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    accuracy(emit)
    emit("%7s %4s %8s | %8s %8s %8s | %7s %6s | %9s %9s %6s | %10s %3s" % (
        "tracks", "H", "mode", "spec med", "gain med", "comp med", "/ comp", "", "spec GB/s", "gain GB/s", "aim",
        "batch us/b", "nb"))
    n = np.arange(N, dtype=np.float64)
    hann = torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * n / N)).astype(np.float32)).cuda()
    S = float(hann.double().sum())
    inv = torch.full((BINS,), 4.0 / (S * S), device="cuda")
    inv[0] = inv[BINS - 1] = 1.0 / (S * S)
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        x = torch.from_numpy(rng.uniform(-1, 1, T * B).astype(np.float32)).cuda()
        z = torch.empty_like(x)
        xs = x.repeat(NB)
        rows = []
        for H in (512, 256):
            per = B // H
            keep = N - H                                   # what the composition carries: the oldest frame's reach
            for mode, bands, name in (("complex", 0, "complex"), ("power", 0, "bins"), ("power", 31, "31 bands")):
                plan = gab.SpectrumPlan(T, B, H, mode, bands)
                if bands:
                    plan.set_bands(gab.spectrum_band_edges(bands))
                out = torch.empty((per, T) + plan.row_shape, device="cuda")
                outs = torch.empty((per * NB, T) + plan.row_shape, device="cuda")
                pargs = plan.prepare(x, out)
                tail = torch.zeros(T, keep, device="cuda")

                def run():
                    plan.launch(pargs)

                def gain():
                    gab.gain(x, 0.5, out=z)

                def comp():
                    both = torch.cat([tail, x.view(T, B)], dim=1)                       # [T, keep + B]
                    fr = torch.stack([both[:, (j + 1) * H + keep - N:(j + 1) * H + keep] for j in range(per)])
                    y = gab.fft_r2c_1024((fr * hann).view(-1), per * T)
                    if mode == "power":
                        y = (y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1]) * inv
                    tail.copy_(both[:, B:])
                    return y

                def batch():
                    plan.process_batch(xs, out=outs)

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
                own = 4.0 * T * B + 4.0 * out.numel()
                rows.append((H, name, float(np.median(t_p)), float(np.median(t_g)), float(np.median(t_c)),
                             float(np.median(t_b)), own))
                plan.close()
                del out, outs, tail
        gains = [r[3] for r in rows]
        margin = (max(gains) - min(gains)) / min(gains)
        for H, name, p, g, c, tb, own in rows:
            r_spec, r_gain = own / (p * 1e-6) / 1e9, 8.0 * T * B / (g * 1e-6) / 1e9
            emit("%7d %4d %8s | %8.2f %8.2f %8.2f | %7.2f %6s | %9.0f %9.0f %6s | %10.2f %3d" % (
                T, H, name, p, g, c, p / c, verdict(p, c, margin), r_spec, r_gain,
                verdict(r_spec, r_gain, margin, lower_is_better=False), tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin" % (
            T, 100.0 * margin, min(gains), max(gains)))
        del x, z, xs
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
