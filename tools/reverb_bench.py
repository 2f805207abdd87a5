#!/usr/bin/env python3
"""Device time of one gab_reverb_process beside gab_gain on the same [T][B] block, in the same process.  B = 512,
O = 2, max_delay = 4096; N = 8 at 8192 and 65536 tracks, N = 4 and N = 16 at 8192 tracks; two sets of delays:
    long   every delay >= 64 (reverb_params' primes from 10 ms): chunks of 64 samples
    short  every delay 32: chunks of 32 samples, half the lanes of the phases along time idle
Every launch is timed by its own pair of HIP events after a warm-up; the median of `--launches` of them and the largest
are reported, the two calls alternated.  process_batch(--batch, 32) is timed the same way and reported per buffer.
Beside the times: the plan's own bytes per buffer, 4 T B (2 N + 1 + O) (x in, y out, N line words in, N out), as a
fraction of 8 TB/s, and the aim: (2 N + 1 + O) / 2 x 1.25 times gain's time, the byte ratio with a quarter on top
because the traffic is N line rows per track rather than one stream.  Met or missed per row.

    python tools/reverb_bench.py [--launches 200] [--out profiles/r15_reverb.txt]

The kernels' own times, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/reverb_bench.py --launches 50

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", default="8192:8,65536:8,8192:4,8192:16", help="tracks:lines, ...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_reverb.txt"))
    args = ap.parse_args()
    B, O, MD, NB = 512, 2, 4096, args.batch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("tools/reverb_bench.py: gab_reverb_process beside gab_gain on the [T][B] block, 512-sample buffers, outs = 2,")
    say("max_delay = 4096; delays long (all >= 64, primes from 10 ms) and short (all 32); process_batch(%d) per buffer;" % NB)
    say("the plan's own bytes 4 T B (2 N + 1 + O) as a fraction of 8 TB/s.  %s, one device, --launches %d: one process,"
        % (torch.cuda.get_device_name(0), args.launches))
    say("every launch between its own pair of HIP events after a warm-up, reverb and gain alternated, median and largest;")
    say("the batch is one launch, median of %d, per buffer.  Times in microseconds.  aim = (2 N + 1 + O) / 2 x 1.25 x the"
        % max(5, args.launches // 20))
    say("gain median of the same row.")
    say("")
    say("%7s %3s %6s | %9s %8s | %8s %8s | %5s %8s %6s | %8s | %10s" % (
        "tracks", "N", "delays", "reverb us", "max us", "gain us", "max us", "x", "aim us", "aim", "of 8TB/s", "batch us/b"))
    for T, N in [tuple(int(v) for v in r.split(":")) for r in args.rows.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z = torch.empty(T * O * B, device="cuda"), torch.empty_like(x)
        xs = x.repeat(NB)
        ys = torch.empty(NB * T * O * B, device="cuda")
        d_long, table = gab.reverb_params(rt60_s=1.0, rt60_hf_s=0.5, size_ms=10.0, lines=N, outs=O)
        assert d_long.min() >= 64 and d_long.max() <= MD
        table = torch.from_numpy(np.tile(table, (T, 1))).cuda()
        for name, d in (("long", d_long), ("short", np.full((1, N), 32, np.int32))):
            plan = gab.ReverbPlan(T, B, lines=N, outs=O, max_delay=MD)
            plan.set_delays(torch.from_numpy(np.ascontiguousarray(np.tile(d, (T, 1)))).cuda())
            plan.set_params(table, ramp=False)
            largs = plan.prepare(x, y)

            def run():
                plan.launch(largs)

            def gain():
                gab.gain(x, 0.5, out=z)

            def batch():
                plan.process_batch(xs, out=ys)

            for _ in range(10):
                run()
                gain()
            batch()
            t_r, t_g, t_b = [], [], []
            for _ in range(args.launches):
                t_r.append(timed(run))
                t_g.append(timed(gain))
            for _ in range(max(5, args.launches // 20)):
                t_b.append(timed(batch) / NB)
            mr, mg, mb = float(np.median(t_r)), float(np.median(t_g)), float(np.median(t_b))
            ratio = (2 * N + 1 + O) / 2.0 * 1.25
            say("%7d %3d %6s | %9.2f %8.2f | %8.2f %8.2f | %5.2f %8.2f %6s | %8.3f | %10.2f" % (
                T, N, name, mr, max(t_r), mg, max(t_g), mr / mg, ratio * mg, "met" if mr <= ratio * mg else "MISSED",
                4.0 * T * B * (2 * N + 1 + O) / (mr * 1e-6) / 8e12, mb))
            assert torch.isfinite(y).all()
            plan.close()
            del plan
    say("")
    say("x: the reverb median over the gain median of the row.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
