"""Long impulse responses on the fdl scheme of the conv plan (gab_conv_create_scheme): device time per buffer of
process() and inside process_batch(n = 32), the scheme's own traffic model against 8 TB/s, the algorithmic bytes of
bench.py / Conv1DAccelBenchmark::algorithmicBytes, the real-time factor, and gab_conv_create's default route (the
direct form above 16384 taps) on the same shapes, each shape of that in a child process under its own time limit.

    python tools/conv_fdl.py [--tracks 128,1024] [--lengths 16384,48000,96000,480000] [--bufsize 512]
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python tools/conv_fdl.py --process-only 1024,512,96000
        (the three launches of a buffer, each kernel's share)
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12                 # bytes/s, the MI355X's nominal HBM bandwidth
BUDGET_MS = 512 / 48000 * 1e3
GROUP, CHUNK, SPREAD_BELOW = 32, 16, 1 << 18      # k_conv_fdl.hip's kGroup, kChunk, kSpreadBelow


def fdl_bytes(T, B, L, n=1):
    """Bytes per buffer the three launches move (reads + writes), at n buffers per MAC launch."""
    K, bins = math.ceil(L / B), B + 1
    plane = T * bins
    G = math.ceil(K / GROUP)
    parts = G if (G > 1 and plane < SPREAD_BELOW) else 1
    fwd = 4 * T * B * 2 + 8 * plane + 4 * T * B / n           # new block (+ the previous), spectrum out, prev copy
    mac = (8 * plane * K + 8 * plane * (K + n - 1)) / n + 8 * plane * parts     # H once, X window, partial sums out
    inv = 8 * plane * parts + 4 * T * B
    return fwd + mac + inv


def ir_on_device(T, L, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(T, L, device="cuda", generator=g) *
            torch.exp(-torch.arange(L, device="cuda", dtype=torch.float32) / (L / 5.0))).contiguous().view(-1)


def time_process(plan, xs, out, count):
    import torch
    ts = []
    for i in range(count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.process(xs[i % len(xs)], out=out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def measure_fdl(T, B, L):
    import numpy as np
    import torch
    import gpuaudiobench_amd as gab
    K = math.ceil(L / B)
    plan = gab.ConvPlan(T, B, L, scheme="fdl")
    t0 = time.time()
    ir = ir_on_device(T, L, 1)
    plan.set_ir(ir)
    torch.cuda.synchronize()
    set_ir_s = time.time() - t0
    del ir
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = torch.randn(32, T * B, device="cuda", generator=g)
    out = torch.empty(T * B, device="cuda")
    for i in range(min(K + CHUNK, 1200)):                 # the delay line fills
        plan.process(xs[i % 32], out=out)
    torch.cuda.synchronize()
    ts = time_process(plan, xs, out, 60)
    xb, ob = xs.view(-1), torch.empty(32 * T * B, device="cuda")
    tb = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.process_batch(xb, 32, out=ob)
        e1.record()
        e1.synchronize()
        tb.append(e0.elapsed_time(e1))
    spectra, history = plan.state_bytes()
    plane = T * (B + 1)
    G = math.ceil(K / GROUP)
    parts = G if (G > 1 and plane < SPREAD_BELOW) else 1
    # beyond state_bytes (taps' spectra + delay line + one previous block): the partial sums, a stateless call's
    # spectrum and the second previous block
    extra = 8 * plane * (CHUNK * parts + 1) + 4 * T * B
    plan.close()
    med, mx = float(np.median(ts)), float(np.max(ts))
    bmed = float(np.median(tb[1:])) / 32
    by1, by32 = fdl_bytes(T, B, L, 1), fdl_bytes(T, B, L, 32 if 32 <= CHUNK else CHUNK)
    alg = 4 * T * (2 * B + 2 * L)
    return {"T": T, "B": B, "L": L, "K": K, "state_gb": round((spectra + history) / 1e9, 3),
            "allocated_gb": round((spectra + history + extra) / 1e9, 3), "set_ir_s": round(set_ir_s, 3),
            "process_ms_median": round(med, 4), "process_ms_max": round(mx, 4),
            "batch32_ms_per_buffer": round(bmed, 4), "batch_speedup": round(med / bmed, 2),
            "fdl_mb_per_buffer": round(by1 / 1e6, 2), "fdl_floor_ms": round(by1 / HBM * 1e3, 4),
            "fdl_frac_of_8tbs": round(by1 / HBM * 1e3 / med, 3),
            "batch_fdl_mb_per_buffer": round(by32 / 1e6, 2), "batch_frac_of_8tbs": round(by32 / HBM * 1e3 / bmed, 3),
            "algorithmic_mb": round(alg / 1e6, 2), "algorithmic_tbs": round(alg / (med * 1e-3) / 1e12, 3),
            "realtime_factor": round(BUDGET_MS / med, 1), "batch_realtime_factor": round(BUDGET_MS / bmed, 1)}


def process_only(T, B, L, count=200):
    """The per-buffer launches alone (for a `rocprofv3 --kernel-trace --stats` pass): the delay line fills, then
    `count` process() calls; prints their median device time."""
    import numpy as np
    import torch
    import gpuaudiobench_amd as gab
    K = math.ceil(L / B)
    plan = gab.ConvPlan(T, B, L, scheme="fdl")
    plan.set_ir(ir_on_device(T, L, 1))
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = torch.randn(32, T * B, device="cuda", generator=g)
    out = torch.empty(T * B, device="cuda")
    for i in range(K + CHUNK):
        plan.process(xs[i % 32], out=out)
    torch.cuda.synchronize()
    ts = time_process(plan, xs, out, count)
    plan.close()
    print(json.dumps({"T": T, "B": B, "L": L, "buffers": count, "process_ms_median": round(float(np.median(ts)), 4)}))


def measure_default_one(T, B, L, count):
    """gab_conv_create's route for the shape: `count` buffers after one untimed one, device time each (child process)."""
    import numpy as np
    import torch
    import gpuaudiobench_amd as gab
    plan = gab.ConvPlan(T, B, L)
    plan.set_ir(ir_on_device(T, L, 1))
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = torch.randn(4, T * B, device="cuda", generator=g)
    out = torch.empty(T * B, device="cuda")
    plan.process(xs[0], out=out)
    torch.cuda.synchronize()
    ts = time_process(plan, xs, out, count)
    plan.close()
    print(json.dumps({"median_ms": float(np.median(ts)), "max_ms": float(np.max(ts))}))


def measure_default(T, B, L, limit_s):
    """A child that runs out of time or ends with any non-zero status (an abort or a fault included) ends the whole
    run: nothing more is started on the GPU after it."""
    route = "uniform" if L <= 16384 else "direct"
    cmd = [sys.executable, os.path.abspath(__file__), "--default-one", "%d,%d,%d" % (T, B, L)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired as e:
        left = (e.stderr or e.stdout or b"")
        left = left.decode("utf-8", "replace") if isinstance(left, bytes) else left
        print("STOP: the default route at T=%d B=%d L=%d ran past %d s; nothing more is started\n%s"
              % (T, B, L, limit_s, left[-2000:]), flush=True)
        sys.exit(124)
    if r.returncode != 0:
        print("STOP: the default route at T=%d B=%d L=%d ended with status %d; nothing more is started\n%s"
              % (T, B, L, r.returncode, (r.stdout + r.stderr)[-2000:]), flush=True)
        sys.exit(1)
    d = json.loads(r.stdout.strip().splitlines()[-1])
    d["route"] = route
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", default="128,1024")
    ap.add_argument("--lengths", default="16384,48000,96000,480000")
    ap.add_argument("--bufsize", type=int, default=512)
    ap.add_argument("--default-one", default=None)
    ap.add_argument("--no-default", action="store_true")
    ap.add_argument("--process-only", default=None, help="T,B,L: per-buffer launches only (under a kernel-trace profiler)")
    a = ap.parse_args()
    if a.process_only:
        process_only(*(int(v) for v in a.process_only.split(",")))
        return
    if a.default_one:
        T, B, L = (int(v) for v in a.default_one.split(","))
        measure_default_one(T, B, L, 5)
        return
    import torch
    print("# device:", torch.cuda.get_device_name(0))
    print("# fdl bytes/buffer = forward (in, prev, spectrum) + MAC (K x H + K x X per buffer; H once per %d-buffer batch"
          " launch) + partial sums + inverse (out); algorithmic = 4 T (2B + 2L)" % CHUNK)
    slow_from = None                 # the shortest response at which the default route took > 1 s per buffer
    for T in sorted(int(v) for v in a.tracks.split(",")):
        for L in sorted(int(v) for v in a.lengths.split(",")):
            row = measure_fdl(T, a.bufsize, L)
            if not a.no_default:
                if slow_from is not None and L >= slow_from:
                    row["default"] = {"skipped": "a response of %d taps already took > 1 s per buffer" % slow_from}
                else:
                    row["default"] = measure_default(T, a.bufsize, L, 240)
                ms = row["default"].get("median_ms")
                if ms is not None and ms > 1000.0:
                    slow_from = L if slow_from is None else min(slow_from, L)
                if ms:
                    row["fdl_speedup_vs_default"] = round(ms / row["process_ms_median"], 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
