#!/usr/bin/env python3
"""Device time of one fused gab_dn_process beside what it replaces, on the same block, in the same process.
B = 512, T in {8192, 65536}, H in {512, 256}, one process and process_batch(--batch, 32).  Every call is timed by its own
pair of HIP events after a warm-up, the four alternated; medians of `--launches` of them are reported (a tenth as many
for the batches), in microseconds per call.

  (a) the yardstick: what a user composes today, SpectrumPlan.process -> the same gate in torch on a carried mask tensor
      -> ResynthesisPlan.process.  Met where the fused call is not slower; a miss by less than 15 % reads "margin"
      (gab_gain's own median moved by 14-15 % between rows of earlier profiles).
  (b) the aim: SpectrumPlan.process + ResynthesisPlan.process with no gate at all.  Met where the fused call takes at
      most that.
  (c) gab_gain on the same block, for scale.

In front of the timings: the accuracy ratios of tests/test_denoise_gpu.py (the fused output's error against the float64
chain over the float32 twin chain's own, per pair, where no decision can flip).

    python tools/denoise_bench.py [--launches 100] [--tracks 8192,65536] [--out profiles/r27_denoise.txt]

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
from spectrum_bench import timed  # noqa: E402

N, BINS = 1024, 513
MARGIN = 0.15


def verdict(value, against, margin=0.0):
    """met: not slower; margin: slower by less than `margin`; else missed."""
    if value <= against:
        return "met"
    return "margin" if value < (1.0 + margin) * against else "missed"


def accuracy(emit):
    import denoise_twin as dt
    import spectrum_twin as st
    emit("# accuracy, T = 3, 4096 samples, B = 512: unit noise under three tones a track, thresholds a factor 1 +- 1e-3")
    emit("# clear of every float64 power, {floor, att, rel} = {0.1, 0.3, 0.7}; per pair, max |y - y64| of the fused")
    emit("# output over that of the float32 twin chain (tests/denoise_twin.py):")
    worst = 0.0
    for H in (256, 512, 100):
        x, thr, params = dt.accuracy_case(3, 4096, H, seed=500 + H)
        ref, P64 = dt.truth64(x, H, thr, params)
        assert dt.clear_of_thresholds(P64, thr, 1e-3)
        twin = dt.Denoiser(3, 4096, H)
        twin.gate.set_thresholds(thr)
        twin.gate.set_params(params)
        e_twin = dt.pair_err(dt.stream_of(twin.process(x[None])), ref)
        plan = gab.DenoisePlan(3, 512, H)
        plan.set_thresholds(torch.from_numpy(thr).cuda())
        plan.set_params(torch.from_numpy(params).cuda())
        y = np.concatenate([plan.process(torch.from_numpy(b).cuda()).cpu().numpy() for b in st.blocks(x, 512)], axis=1)
        plan.close()
        ratio = dt.pair_err(y, ref) / e_twin
        worst = max(worst, float(ratio.max()))
        emit("#   H %3d  e_twin %s  ratio %s" % (H, " ".join("%.3g" % v for v in e_twin), " ".join("%.2f" % v for v in ratio)))
    emit("# largest ratio %.2f: %s the factor 4 of tests/test_resynthesis_gpu.py" % (
        worst, "inside" if worst <= 4.0 else "ABOVE"))


class TorchGate:
    """The header's gate in torch on a carried mask tensor [T][513]: a frame at a time, in order."""

    def __init__(self, T, thr, params, inv):
        self.mask = torch.ones(T, BINS, device="cuda")
        self.thr, self.inv = thr, inv
        self.floor, self.att, self.rel = (params[:, i:i + 1].contiguous() for i in range(3))
        self.one = torch.ones((), device="cuda")

    def __call__(self, rows):
        for j in range(rows.shape[0]):
            r = rows[j]
            P = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) * self.inv
            tg = torch.where(P > self.thr, self.one, self.floor)
            c = torch.where(tg > self.mask, self.att, self.rel)
            self.mask = torch.addcmul(tg, c, self.mask - tg)
            r *= self.mask[..., None]
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_denoise.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/denoise_bench.py --launches %d --batch %d: %s, medians in microseconds per call" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    accuracy(emit)
    emit("%7s %4s %3s | %9s | %9s %7s %6s | %9s %7s %6s | %8s" % (
        "tracks", "H", "nb", "fused", "(a) comp", "/ (a)", "", "(b) plain", "/ (b)", "", "(c) gain"))
    S = float(np.sum(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)))
    inv = torch.full((BINS,), 4.0 / (S * S), device="cuda")
    inv[0] = inv[BINS - 1] = 1.0 / (S * S)
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        thr = torch.from_numpy((0.002 * 10.0 ** rng.uniform(-1, 1, (T, BINS))).astype(np.float32)).cuda()
        params = torch.from_numpy(np.tile(gab.denoise_params(hop=256), (T, 1))).cuda()
        for H in (512, 256):
            for nb in (1, NB):
                xs = torch.from_numpy(rng.uniform(-1, 1, nb * T * B).astype(np.float32)).cuda().view(nb, T, B)
                out, z = torch.empty_like(xs), torch.empty_like(xs)
                fused = gab.DenoisePlan(T, B, H)
                spec, resyn = gab.SpectrumPlan(T, B, H, "complex"), gab.ResynthesisPlan(T, B, H)
                fused.set_thresholds(thr)
                fused.set_params(params)
                gate = TorchGate(T, thr, params, inv)
                rows = torch.empty((nb * B // H, T, BINS, 2), device="cuda")
                y = torch.empty_like(xs)

                def run():
                    fused.process_batch(xs, out=out) if nb > 1 else fused.process(xs, out=out)

                def analyse():
                    return spec.process_batch(xs, out=rows) if nb > 1 else spec.process(xs, out=rows)

                def synth(r):
                    resyn.process_batch(r, nb, out=y) if nb > 1 else resyn.process(r, out=y)

                def comp():
                    synth(gate(analyse()))

                def plain():
                    synth(analyse())

                def gain():
                    gab.gain(xs, 0.5, out=z)

                for _ in range(3):
                    run(), comp(), plain(), gain()
                t = {k: [] for k in "fabc"}
                for _ in range(args.launches if nb == 1 else max(5, args.launches // 10)):
                    t["f"].append(timed(run))
                    t["a"].append(timed(comp))
                    t["b"].append(timed(plain))
                    t["c"].append(timed(gain))
                f, a, b, c = (float(np.median(t[k])) for k in "fabc")
                emit("%7d %4d %3d | %9.1f | %9.1f %7.2f %6s | %9.1f %7.2f %6s | %8.1f" % (
                    T, H, nb, f, a, f / a, verdict(f, a, MARGIN), b, f / b, verdict(f, b), c))
                for p in (fused, spec, resyn):
                    p.close()
                del xs, out, z, rows, y, gate
                torch.cuda.empty_cache()
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
