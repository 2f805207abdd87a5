#!/usr/bin/env python3
"""Device time of one gab_fdaf_process and of process_batch(--batch, 32), 512-sample buffers, adapting (mu = 0.5 at
K = 1, else 1; a floor of -60 dB; the input holds an echo of the reference under noise).  Rows: 8192 and 65536 tracks
at K = 1 and 4, 1024 and 8192 tracks at K = 16 (a row whose state does not fit the free memory is reported as left out).
Every launch is timed by its own pair of HIP events after a warm-up, the plan alternated with its references in one
process on one box; medians (p99 and largest for the plan's own launch).  A yardstick counts as met inside its own
spread, the interquartile range of its launches.  Reported per row, none enforced:

  (a) the yardstick: not slower than what a user composes today, the same seven steps in torch (torch.fft.rfft / irfft
      on [T][K][513] tensors), timed in the same loop at the same shape (at 65536 tracks it is run at 8192 tracks and
      scaled by 8: its temporaries would not fit beside the plan's state);
  (b) at K = 1: not slower than NlmsPlan(taps=512) adapting on the same blocks; the ratio at every K;
  (c) the aim: 8192 tracks at K = 16 in one process inside the 10 667 us slot of a 512-sample buffer at 48 kHz;
  (d) the launch's own bytes, 5 K 4104 B a track and block for the two passes and the write of W plus the four blocks
      (8192 B a track), over its time, as a fraction of 8 TB/s; and gab_gain on the same block.

    python tools/fdaf_bench.py [--launches 30] [--out profiles/r32_fdaf.txt]

The kernel's own time, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/fdaf_bench.py --launches 10 --out /dev/null
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpuaudiobench_amd as gab  # noqa: E402

SLOT_US = 512 / 48000.0 * 1e6
HBM_BYTES_PER_US = 8e12 / 1e6
ROWS = ((8192, 1), (65536, 1), (8192, 4), (65536, 4), (1024, 16), (8192, 16))


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


def signals(T, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 0.25 * torch.randn(T, n, device="cuda", generator=g)
    d = 0.01 * torch.randn(T, n, device="cuda", generator=g)
    d[:, 3:] += 0.5 * x[:, :-3]
    return d.reshape(-1).contiguous(), x.reshape(-1).contiguous()


class TorchFdaf:
    """The header's seven steps as a user composes them: a track alone in its transforms, torch.fft, no skip."""

    def __init__(self, T, K, mu, eps):
        self.T, self.K, self.mu, self.eps = T, K, mu, eps
        self.W = torch.zeros(T, K, 513, dtype=torch.complex64, device="cuda")
        self.X = torch.zeros_like(self.W)
        self.prev = torch.zeros(T, 512, device="cuda")
        self.count = 0

    def block(self, d, x, err):
        K, slot = self.K, self.count % self.K
        self.X[:, slot] = torch.fft.rfft(torch.cat([self.prev, x], dim=1), dim=1)
        order = [(slot - p) % K for p in range(K)]
        Xs = self.X[:, order]
        Y = (Xs * self.W).sum(1)
        S = (Xs.real * Xs.real + Xs.imag * Xs.imag).sum(1)
        est = torch.fft.irfft(Y, n=1024, dim=1)[:, 512:]
        torch.sub(d, est, out=err)
        E = torch.fft.rfft(torch.nn.functional.pad(err, (512, 0)), dim=1)
        G = (self.mu / (S + self.eps)) * E
        self.W += Xs.conj() * G[:, None]
        w = torch.fft.irfft(self.W[:, slot], n=1024, dim=1)
        w[:, 512:] = 0
        self.W[:, slot] = torch.fft.rfft(w, dim=1)
        self.prev = x
        self.count += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--torch-tracks", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_fdaf.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/fdaf_bench.py --launches %d --batch %d: %s, %d CUs, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count))
    emit("%7s %3s %6s | %9s %9s %9s | %10s %3s | %9s %7s | %9s %7s | %8s %6s | %9s | %s" % (
        "tracks", "K", "taps", "fdaf med", "p99", "max", "batch us/b", "nb", "torch (a)", "fdaf/a", "nlms512", "fdaf/b",
        "MB", "of HBM", "gain", "verdicts"))
    for T, K in ROWS:
        # the plan's W and X; the composed form's W and X and its temporaries of that size (the gathered delay line, two
        # products, the conjugate) at its own track count; NlmsPlan's taps and history; three batches and their making
        Tc = min(T, args.torch_tracks)
        need = 2 * T * K * 513 * 8 + 6 * Tc * K * 513 * 8 + 2 * T * 512 * 4 + 6 * NB * T * B * 4
        free = torch.cuda.mem_get_info()[0]
        if need > 0.8 * free:
            emit("%7d %3d %6d | left out: %.1f GB of state, temporaries and blocks against %.1f GB free" % (
                T, K, 512 * K, need / 1e9, free / 1e9))
            continue
        mu = 0.5 if K == 1 else 1.0
        row = gab.fdaf_params(mu, -60.0, K)
        d, x = signals(T, B, 1)
        e, z = torch.empty_like(d), torch.empty_like(d)
        ds, xs = signals(T, NB * B, 2)
        ds = ds.view(T, NB, B).transpose(0, 1).contiguous().view(-1)
        xs = xs.view(T, NB, B).transpose(0, 1).contiguous().view(-1)
        es = torch.empty_like(ds)
        plan, nlms = gab.FdafPlan(T, B, K), gab.NlmsPlan(T, B, 512)
        plan.set_params(torch.from_numpy(np.tile(row, (T, 1))).cuda())
        nlms.set_params(torch.from_numpy(np.tile(gab.nlms_params(0.5, -60.0, 512), (T, 1))).cuda(), ramp=False)
        pargs, nargs = plan.prepare(d, x, err=e), nlms.prepare(d, x, err=z)
        Tt = min(T, args.torch_tracks)
        composed = TorchFdaf(Tt, K, float(row[0]), float(row[1]))
        dt, xt, et = d.view(T, B)[:Tt], x.view(T, B)[:Tt], torch.empty(Tt, B, device="cuda")
        calls = {"fdaf": lambda: plan.launch(pargs), "torch": lambda: composed.block(dt, xt, et),
                 "nlms": lambda: nlms.launch(nargs), "gain": lambda: gab.gain(d, 0.5, out=z)}
        for _ in range(K + 3):                                       # the delay line fills
            for fn in calls.values():
                fn()
        plan.process_batch(ds, xs, err=es)
        t = {k: [] for k in calls}
        for _ in range(args.launches):
            for k, fn in calls.items():                               # alternated
                t[k].append(timed(fn))
        t_b = [timed(lambda: plan.process_batch(ds, xs, err=es)) / NB for _ in range(max(3, args.launches // 10))]
        p, a, n = stats(t["fdaf"]), stats(t["torch"]), stats(t["nlms"])
        a_med = a[0] * (T / Tt)
        verdicts = ["(a) %s" % ("met" if p[0] <= a_med * (1 + iqr(t["torch"])) else "MISSED")]
        if K == 1:
            verdicts.append("(b) %s" % ("met" if p[0] <= n[0] * (1 + iqr(t["nlms"])) else "MISSED"))
        if (T, K) == (8192, 16):
            verdicts.append("(c) %s (%.2f of the slot)" % ("met" if p[0] <= SLOT_US else "MISSED", p[0] / SLOT_US))
        nbytes = T * (5 * K * 4104 + 4 * B * 4)
        emit("%7d %3d %6d | %9.1f %9.1f %9.1f | %10.1f %3d | %9.1f %7.4f | %9.1f %7.3f | %8.1f %6.3f | %9.1f | %s" % (
            T, K, 512 * K, p[0], p[1], p[2], float(np.median(t_b)), NB, a_med, p[0] / a_med, n[0], p[0] / n[0],
            nbytes / 1e6, nbytes / p[0] / HBM_BYTES_PER_US, float(np.median(t["gain"])), ", ".join(verdicts)))
        plan.close()
        nlms.close()
        del composed, plan, nlms, d, x, e, z, ds, xs, es, dt, xt, et
        torch.cuda.empty_cache()
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
