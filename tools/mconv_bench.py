#!/usr/bin/env python3
"""Device time of one gab_mconv_process and of process_batch(--batch, 32) per buffer, 512-sample buffers, steady (no
ramp pending), decaying random taps.  Rows (inputs, outputs, K): (1024, 2, 1), (4096, 2, 1), (256, 16, 2), (64, 64, 4),
(2, 2, 32).  Every call is timed by its own pair of HIP events after a warm-up, the plan alternated with its references
in one process on one box; medians (p99 and largest for the plan's own call).  A yardstick counts as met inside its own
spread, the interquartile range of its launches.  Reported per row, none enforced:

  (a) not slower than what a user composes today in this library: per output an FdafPlan(inputs, K) with mu = 0 and that
      output's taps, est only, then a MixPlan(inputs -> 1) at unit gain: 2 O launches a buffer;
  (b) not slower than the same three steps in torch: torch.fft.rfft of the windows, an einsum over a ring tensor,
      torch.fft.irfft;
  (c) the aim, recorded: the product launch's own bytes (H once, the K slots of X, the partials) over the WHOLE call's
      time as a fraction of 8 TB/s, a floor on what the product launch itself reaches (its own time: the rocprofv3
      line below); and gab_gain on the input block.

    python tools/mconv_bench.py [--launches 20] [--out profiles/r33_mconv.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/mconv_bench.py --launches 10 --plan-only --out /dev/null
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpuaudiobench_amd as gab  # noqa: E402

HBM_BYTES_PER_US = 8e12 / 1e6
ROWS = ((1024, 2, 1), (4096, 2, 1), (256, 16, 2), (64, 64, 4), (2, 2, 32))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(t):
    return float(np.median(t)), float(np.percentile(t, 99)), float(max(t))


def iqr(t):
    """A yardstick's own spread: the interquartile range of its launches over their median (an outlier does not move it)."""
    return float((np.percentile(t, 75) - np.percentile(t, 25)) / np.median(t))


def taps(O, I, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.arange(512 * K, device="cuda")
    return (0.2 * torch.randn(O, I, 512 * K, device="cuda", generator=g) * torch.exp(-n / (100.0 * K))).contiguous()


class Composed:
    """Yardstick (a): O x (FdafPlan with mu = 0, est only -> MixPlan to one bus at unit gain)."""

    def __init__(self, I, O, K, B, h):
        self.filters = [gab.FdafPlan(I, B, K) for _ in range(O)]
        self.mixes = [gab.MixPlan(I, B, 1) for _ in range(O)]
        ones = torch.ones(I, 1, device="cuda")
        for o in range(O):
            self.filters[o].set_taps(h[o].contiguous())
            self.mixes[o].set_gains(ones, ramp=False)
        self.est = torch.empty(I * B, device="cuda")
        self.B = B

    def process(self, x, y):
        for o, (f, m) in enumerate(zip(self.filters, self.mixes)):
            f.process(x, x, est=self.est)
            m.process(self.est, out=y[o * self.B:(o + 1) * self.B])

    def close(self):
        for p in self.filters + self.mixes:
            p.close()


class TorchMconv:
    """Yardstick (b): rfft of the windows, an einsum over a ring tensor, irfft."""

    def __init__(self, I, O, K, h):
        h = h.view(O, I, K, 512)
        self.H = torch.fft.rfft(torch.nn.functional.pad(h, (0, 512)), dim=-1)         # [O][I][K][513]
        self.ring = torch.zeros(K, I, 513, dtype=torch.complex64, device="cuda")
        self.prev = torch.zeros(I, 512, device="cuda")
        self.K, self.count = K, 0

    def process(self, x, y):
        slot = self.count % self.K
        self.ring[slot] = torch.fft.rfft(torch.cat([self.prev, x], dim=1), dim=1)
        order = [(slot - p) % self.K for p in range(self.K)]
        Y = torch.einsum("pik,oipk->ok", self.ring[order], self.H)
        y.copy_(torch.fft.irfft(Y, n=1024, dim=1)[:, 512:])
        self.prev = x
        self.count += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--plan-only", action="store_true", help="the plan's own calls alone (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_mconv.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/mconv_bench.py --launches %d --batch %d: %s, %d CUs, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    emit("%6s %3s %3s %6s | %9s %9s %9s | %10s %3s | %11s %8s | %9s %8s | %8s %6s | %8s | %s" % (
        "inputs", "out", "K", "taps", "mconv med", "p99", "max", "batch us/b", "nb", "composed(a)", "mconv/a", "torch (b)",
        "mconv/b", "MB", "of HBM", "gain", "verdicts"))
    for I, O, K in ROWS:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = 0.25 * torch.randn(I * B, device="cuda", generator=g)
        xs = 0.25 * torch.randn(NB * I * B, device="cuda", generator=g)
        y, ys, z = torch.empty(O * B, device="cuda"), torch.empty(NB * O * B, device="cuda"), torch.empty(I * B, device="cuda")
        h = taps(O, I, K, 2)
        plan = gab.MatrixConvPlan(I, O, B, K)
        plan.set_taps(h, ramp=False)
        pargs = plan.prepare(x, y)
        calls = {"mconv": lambda: plan.launch(pargs)}
        if not args.plan_only:
            composed, composed_y = Composed(I, O, K, B, h), torch.empty(O * B, device="cuda")
            torched, torch_y = TorchMconv(I, O, K, h), torch.empty(O, B, device="cuda")
            calls.update({"composed": lambda: composed.process(x, composed_y),
                          "torch": lambda: torched.process(x.view(I, B), torch_y),
                          "gain": lambda: gab.gain(x, 0.5, out=z)})
        for _ in range(K + 3):                                       # the ring fills
            for fn in calls.values():
                fn()
        plan.process_batch(xs, out=ys)
        t = {k: [] for k in calls}
        for _ in range(args.launches):
            for k, fn in calls.items():                               # alternated
                t[k].append(timed(fn))
        t_b = [timed(lambda: plan.process_batch(xs, out=ys)) / NB for _ in range(max(3, args.launches // 5))]
        p = stats(t["mconv"])
        G = (I + 31) // 32
        nbytes = 4104 * (O * I * K + K * I + O * G)
        if args.plan_only:
            emit("%6d %3d %3d %6d | %9.1f %9.1f %9.1f | %10.1f %3d" % (I, O, K, 512 * K, p[0], p[1], p[2],
                                                                       float(np.median(t_b)), NB))
        else:
            a, b = stats(t["composed"]), stats(t["torch"])
            verdicts = ["(a) %s" % ("met" if p[0] <= a[0] * (1 + iqr(t["composed"])) else "MISSED"),
                        "(b) %s" % ("met" if p[0] <= b[0] * (1 + iqr(t["torch"])) else "MISSED")]
            emit("%6d %3d %3d %6d | %9.1f %9.1f %9.1f | %10.1f %3d | %11.1f %8.4f | %9.1f %8.4f | %8.1f %6.3f | %8.1f | %s" % (
                I, O, K, 512 * K, p[0], p[1], p[2], float(np.median(t_b)), NB, a[0], p[0] / a[0], b[0], p[0] / b[0],
                nbytes / 1e6, nbytes / p[0] / HBM_BYTES_PER_US, float(np.median(t["gain"])), ", ".join(verdicts)))
            composed.close()
            del composed, torched
        plan.close()
        del plan, x, xs, y, ys, z, h
        torch.cuda.empty_cache()
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
