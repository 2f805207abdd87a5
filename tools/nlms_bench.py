#!/usr/bin/env python3
"""Device time of one gab_nlms_process and of process_batch(--batch, 32), 512-sample buffers, T in {8192, 65536},
L in {64, 512}, adapting (mu = 0.5, a floor of -60 dB; the input holds an echo of the reference under noise).
Every launch is timed by its own pair of HIP events after a warm-up, the plan alternated with each reference on one
box; medians (p99 and largest for the plan's own launch).  Four things are reported per row and none is enforced:

  (a) the yardstick: not slower than what a user composes today, the same recursion in torch on [T][L] tensors, one
      sample at a time (a roll, two products, two sums, a division, an addcmul: some ten launches a sample).  It is run
      at --torch-tracks (8192) tracks for --torch-samples (64) samples, alternated with the plan at that track count,
      and scaled to the 512 samples of a buffer;
  (b) the aim: one process at 65 536 tracks and L = 512 inside the 10 667 us slot of a 512-sample buffer at 48 kHz;
  (c) a count floor beside it: the 3 R fmaf per sample and lane (two chains and the update), at 2 cycles per wave64
      v_fma_f32 with several waves on a SIMD, times the waves a SIMD is given (tracks / (4 CUs), rounded up), at the
      clock the device reports; and the ratio of the measured time to it;
  (d) informative, at mu = 0 (the plan as a per-track FIR filter): gab_conv1d at the same taps where it takes the shape,
      and gab_gain on the block.

    python tools/nlms_bench.py [--launches 30] [--tracks 8192,65536] [--out profiles/r31_nlms.txt]

The kernel's own time, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/nlms_bench.py --launches 10 --out /dev/null
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(t):
    return float(np.median(t)), float(np.percentile(t, 99)), float(max(t))


def clock_mhz():
    """The device's peak shader clock, from the runtime (hipDeviceAttributeClockRate, kHz)."""
    import ctypes
    khz = ctypes.c_int(0)
    rc = ctypes.CDLL("libamdhip64.so").hipDeviceGetAttribute(ctypes.byref(khz), 5, torch.cuda.current_device())
    assert rc == 0 and khz.value > 0, rc
    return khz.value / 1e3


def signals(T, B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 0.25 * torch.randn(T, B, device="cuda", generator=g)
    d = 0.01 * torch.randn(T, B, device="cuda", generator=g)
    d[:, 3:] += 0.5 * x[:, :-3]
    return d.reshape(-1).contiguous(), x.reshape(-1).contiguous()


def torch_nlms(w, X, d, x, err, mu, eps, n):
    """The recursion as a user composes it: w, X [T][L]; d, x, err [T][B]; n samples."""
    for s in range(n):
        X = torch.roll(X, 1, 1)
        X[:, 0] = x[:, s]
        y = (w * X).sum(1)
        e = d[:, s] - y
        g = mu / ((X * X).sum(1) + eps) * e
        w.addcmul_(g[:, None], X)
        err[:, s] = e
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--tracks", default="8192,65536")
    ap.add_argument("--taps", default="64,512")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--torch-tracks", type=int, default=8192)
    ap.add_argument("--torch-samples", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_nlms.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    cus, mhz = torch.cuda.get_device_properties(0).multi_processor_count, clock_mhz()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/nlms_bench.py --launches %d --batch %d: %s, %d CUs at %.0f MHz, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0), cus, mhz))
    emit("%7s %4s | %9s %9s %9s | %10s %3s | %9s %6s | %9s %9s %9s | %s" % (
        "tracks", "L", "nlms med", "p99", "max", "batch us/b", "nb", "floor (c)", "ratio", "mu=0 med", "conv1d", "gain",
        "aim (b): one process within %.0f us" % SLOT_US))
    for T in [int(v) for v in args.tracks.split(",")]:
        d, x = signals(T, B, 1)
        e, z = torch.empty_like(d), torch.empty_like(d)
        ds, xs = d.repeat(NB), x.repeat(NB)
        es = torch.empty_like(ds)
        for L in [int(v) for v in args.taps.split(",")]:
            R = L // 64
            plan, fir = gab.NlmsPlan(T, B, L), gab.NlmsPlan(T, B, L)
            plan.set_params(torch.from_numpy(np.tile(gab.nlms_params(0.5, -60.0, L), (T, 1))).cuda(), ramp=False)
            taps = (0.05 * torch.randn(T, L, device="cuda")).contiguous()
            fir.set_taps(taps)                                        # mu = 0: the per-track FIR filter
            pargs, fargs = plan.prepare(d, x, err=e), fir.prepare(d, x, est=z)
            conv_ok = True
            try:
                gab.conv1d(x, taps.reshape(-1), L, T, B)
            except gab.GabError:
                conv_ok = False
            calls = {"nlms": lambda: plan.launch(pargs), "fir": lambda: fir.launch(fargs),
                     "gain": lambda: gab.gain(d, 0.5, out=z)}
            if conv_ok:
                calls["conv1d"] = lambda: gab.conv1d(x, taps.reshape(-1), L, T, B)
            for _ in range(3):
                for fn in calls.values():
                    fn()
            plan.process_batch(ds, xs, err=es)
            t = {k: [] for k in calls}
            for _ in range(args.launches):
                for k, fn in calls.items():                           # alternated
                    t[k].append(timed(fn))
            t_b = [timed(lambda: plan.process_batch(ds, xs, err=es)) / NB for _ in range(max(3, args.launches // 10))]
            p = stats(t["nlms"])
            floor = 3.0 * R * 2.0 * B * -(-T // (4 * cus)) / mhz
            aim = ""
            if T == 65536 and L == 512:
                aim = "%s (%.2f of the slot)" % ("met" if p[0] <= SLOT_US else "MISSED", p[0] / SLOT_US)
            emit("%7d %4d | %9.1f %9.1f %9.1f | %10.1f %3d | %9.1f %6.2f | %9.1f %9s %9.1f | %s" % (
                T, L, p[0], p[1], p[2], float(np.median(t_b)), NB, floor, p[0] / floor, float(np.median(t["fir"])),
                "%.1f" % float(np.median(t["conv1d"])) if conv_ok else "refused", float(np.median(t["gain"])), aim))
            plan.close()
            fir.close()
        del d, x, e, z, ds, xs, es
    # (a) the composed form
    T, n = args.torch_tracks, args.torch_samples
    d, x = signals(T, B, 2)
    e = torch.empty_like(d)
    for L in [int(v) for v in args.taps.split(",")]:
        plan = gab.NlmsPlan(T, B, L)
        row = gab.nlms_params(0.5, -60.0, L)
        plan.set_params(torch.from_numpy(np.tile(row, (T, 1))).cuda(), ramp=False)
        pargs = plan.prepare(d, x, err=e)
        w, X = torch.zeros(T, L, device="cuda"), torch.zeros(T, L, device="cuda")
        te = torch.empty(T, B, device="cuda")
        mu, eps = float(row[0]), float(row[1])
        state = [X]

        def composed():
            state[0] = torch_nlms(w, state[0], d.view(T, B), x.view(T, B), te, mu, eps, n)

        composed()
        plan.launch(pargs)
        t_c, t_p = [], []
        for _ in range(max(3, args.launches // 6)):
            t_c.append(timed(composed) * (B / n))
            t_p.append(timed(lambda: plan.launch(pargs)))
        c, p = float(np.median(t_c)), float(np.median(t_p))
        emit("# (a) %d tracks, L = %d: torch, one sample at a time, %d samples scaled to %d: %.0f us a buffer; the plan "
             "%.1f us (%.4f of it): %s" % (T, L, n, B, c, p, p / c, "met" if p <= c else "MISSED"))
        plan.close()
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
