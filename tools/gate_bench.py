#!/usr/bin/env python3
"""Device time of one gab_gate_process beside gab_gain and gab_dyn_process on the same block, in the same process.
B = 512, T in {8192, 65536}; a steady buffer and a ramp buffer, with and without a key block, a hold of 0 and one longer
than the buffer.  The tracks gate: noise whose level steps between full scale and -40 dB every 128 samples, open at
-20 dB, close at -26 dB, attack 1 ms, release 100 ms.
Every launch is timed by its own pair of HIP events after a warm-up, the three calls alternated; median, p99 and
largest of `--launches` of them are reported.  On a ramp row a ramped set_params (synchronous, outside the timed pair)
precedes every gate launch.  process_batch(--batch, 32) is timed the same way and reported per buffer (on a ramp row
the ramp runs through the first of its buffers).  The plan moves 8 T B bytes per buffer (x in, y out), 12 T B with a
key; gab_gain moves 8 T B.  Two yardsticks, reported and not enforced: the dynamics plan's median from the same row
(the gate does less arithmetic per sample and should not be slower), and gab_gain's median from the same row scaled
by the bytes (x 12 / 8 with a key).  The margin of both comparisons is the spread of gab_gain's own median over the
rows of one track count, printed below each group.

    python tools/gate_bench.py [--launches 200] [--tracks 8192,65536] [--out profiles/r17_gate.txt]

The kernels' own times, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/gate_bench.py --launches 50 --out /dev/null

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_gate.txt"))
    args = ap.parse_args()
    B, NB = 512, args.batch
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# tools/gate_bench.py --launches %d --batch %d: %s, times in microseconds" % (
        args.launches, NB, torch.cuda.get_device_name(0)))
    emit("%7s %6s %4s %5s | %8s %8s %8s | %8s %8s | %8s %8s | %8s %4s | %8s %4s %8s | %10s %3s" % (
        "tracks", "buffer", "key", "hold", "gate med", "p99", "max", "gain med", "p99", "dyn med", "p99",
        "<= dyn", "met", "aim", "met", "of 8TB/s", "batch us/b", "nb"))
    for T in [int(v) for v in args.tracks.split(",")]:
        rng = np.random.RandomState(1)
        env = np.repeat(rng.choice([1.0, 0.01], size=(T, B // 128)), 128, axis=1).ravel()
        x = torch.from_numpy((rng.uniform(-1, 1, T * B) * env).astype(np.float32)).cuda()
        k = torch.from_numpy((rng.uniform(-1, 1, T * B) * env[::-1]).astype(np.float32)).cuda()
        y, z, w = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        xs, ks = x.repeat(NB), k.repeat(NB)
        ys = torch.empty_like(xs)
        dyn = gab.DynamicsPlan(T, B, 1)
        dyn.set_params(torch.from_numpy(np.tile(gab.dynamics_params(-18.0, 4.0, 0.0, 5.0, 100.0, makeup_db=3.0),
                                                (T, 1))).cuda(), ramp=False)
        rows = []
        for ramped in (False, True):
            for keyed in (False, True):
                for hold_ms in (0.0, 1000.0 * 2 * B / 48000.0):
                    plan = gab.GatePlan(T, B, 1)
                    row = gab.gate_params(-20.0, close_db=-26.0, attack_ms=1.0, release_ms=100.0, hold_ms=hold_ms,
                                          range_db=-60.0)
                    other = gab.gate_params(-24.0, close_db=-30.0, attack_ms=2.0, release_ms=50.0, hold_ms=hold_ms,
                                            range_db=-40.0)
                    tabs = [torch.from_numpy(np.tile(r, (T, 1))).cuda() for r in (row, other)]
                    plan.set_params(tabs[0], ramp=False)
                    largs = plan.prepare(x, y, key=k if keyed else None)
                    dargs = dyn.prepare(x, w, key=k if keyed else None)
                    turn = [0]

                    def arm():
                        if ramped:
                            turn[0] ^= 1
                            plan.set_params(tabs[turn[0]], ramp=True)

                    def run():
                        plan.launch(largs)

                    def gain():
                        gab.gain(x, 0.5, out=z)

                    def dyn1():
                        dyn.launch(dargs)

                    def batch():
                        plan.process_batch(xs, key=ks if keyed else None, out=ys)

                    for _ in range(10):
                        arm()
                        run()
                        gain()
                        dyn1()
                    arm()
                    batch()
                    t_p, t_g, t_d, t_b = [], [], [], []
                    for _ in range(args.launches):
                        arm()
                        t_p.append(timed(run))
                        t_g.append(timed(gain))
                        t_d.append(timed(dyn1))
                    for _ in range(max(5, args.launches // 20)):
                        arm()
                        t_b.append(timed(batch) / NB)
                    p, g, d = stats(t_p), stats(t_g), stats(t_d)
                    nbytes = (12.0 if keyed else 8.0) * T * B
                    aim = g[0] * nbytes / (8.0 * T * B)
                    rows.append((ramped, keyed, hold_ms, p, g, d, aim, nbytes, float(np.median(t_b))))
                    plan.close()
        gains = [r[4][0] for r in rows]
        margin = (max(gains) - min(gains)) / min(gains)
        slower = sum(1 for r in rows if r[3][0] > r[5][0] * (1.0 + margin))
        missed = sum(1 for r in rows if r[3][0] > r[6] * (1.0 + margin))
        for ramped, keyed, hold_ms, p, g, d, aim, nbytes, tb in rows:
            emit("%7d %6s %4s %5d | %8.2f %8.2f %8.2f | %8.2f %8.2f | %8.2f %8.2f | %8.2f %4s | %8.2f %4s %8.3f | %10.2f %3d" % (
                T, "ramp" if ramped else "steady", "yes" if keyed else "no", int(round(hold_ms * 48.0)), p[0], p[1], p[2],
                g[0], g[1], d[0], d[1], p[0] / d[0], "yes" if p[0] <= d[0] * (1.0 + margin) else "no", aim,
                "yes" if p[0] <= aim * (1.0 + margin) else "no", nbytes / (p[0] * 1e-6) / 8e12, tb, NB))
        emit("# %d tracks: gab_gain's median moved by %.1f %% between these rows (%.2f .. %.2f us): the margin of `met`" % (
            T, 100.0 * margin, min(gains), max(gains)))
        emit("# %d tracks: slower than the dynamics plan in %d of %d rows; the aim (gab_gain scaled by the bytes) MISSED in "
             "%d of %d rows, by %.2f x to %.2f x" % (T, slower, len(rows), missed, len(rows),
                                                   min(r[3][0] / r[6] for r in rows), max(r[3][0] / r[6] for r in rows)))
        dyn.close()
        del x, k, y, z, w, xs, ks, ys
    if args.out and args.out != os.devnull:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
