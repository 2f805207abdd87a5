#!/usr/bin/env python3
"""Device time of one gab_eq_process beside what the library could do before it: S successive gab_iir launches over
the same block.  T in {128, 1024, 8192, 65536}, B = 512, S in {1, 2, 4, 8, 16}; HIP events around `--launches` launches
of each after a warm-up, the two alternated in the same process.  Beside the times: the fused kernel's own bytes
(2 T B 4 + T S (table row + 16)) and the fraction of 8 TB/s they come to.

    python tools/eq_bench.py [--launches 200] [--tracks 128,1024,8192,65536] [--sections 1,2,4,8,16]

The kernel's own time, in a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/eq_bench.py --launches 50

The outputs at these shapes: tests/test_scale_gpu.py::test_bench_shape (bits, against per-buffer calls and a shard).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpuaudiobench_amd as gab  # noqa: E402

FS = 48000.0


def bank(T, S, seed):
    """Stable sections: a 12 dB/oct high-pass, then RBJ peaking sections (what tests/test_eq_host.py's banks are)."""
    rng = np.random.RandomState(seed)
    f = np.where(np.arange(S)[None, :] == 0, 240.0 * 4.0 ** rng.uniform(size=(T, S)), 240.0 * (16000.0 / 240.0) ** rng.uniform(size=(T, S)))
    q = np.where(np.arange(S)[None, :] == 0, np.sqrt(0.5), 0.5 * 16.0 ** rng.uniform(size=(T, S)))
    A = np.where(np.arange(S)[None, :] == 0, 1.0, 10.0 ** (rng.uniform(-12.0, 12.0, size=(T, S)) / 40.0))
    w0 = 2.0 * np.pi * f / FS
    al, c = np.sin(w0) / (2.0 * q), np.cos(w0)
    hp = np.arange(S)[None, :] == 0
    b0 = np.where(hp, (1 + c) / 2, 1 + al * A)
    b1 = np.where(hp, -(1 + c), -2 * c)
    b2 = np.where(hp, (1 + c) / 2, 1 - al * A)
    a0 = np.where(hp, 1 + al, 1 + al / A)
    a2 = np.where(hp, 1 - al, 1 - al / A)
    return (np.stack([b0, b1, b2, -2 * c, a2], axis=-1) / a0[..., None]).astype(np.float32)


def events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--tracks", default="128,1024,8192,65536")
    ap.add_argument("--sections", default="1,2,4,8,16")
    args = ap.parse_args()
    B = 512
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    iir_c = (C.c_float * 5)(0.2, 0.1, -0.05, -1.2, 0.72)
    print("%7s %3s %6s | %9s %9s %6s | %9s %8s" % ("tracks", "S", "form", "eq us", "S x iir", "ratio", "eq bytes", "of 8TB/s"))
    for T in [int(v) for v in args.tracks.split(",")]:
        x = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, T * B).astype(np.float32)).cuda()
        y, z = torch.empty_like(x), torch.empty_like(x)
        st = torch.zeros(2 * T, device="cuda")
        px, py, pz, pst = (C.c_void_p(t.data_ptr()) for t in (x, y, z, st))
        for S in [int(v) for v in args.sections.split(",")]:
            plan = gab.EqPlan(T, B, S)
            plan.set_coeffs(torch.from_numpy(bank(T, S, 3)).cuda())
            eq_args = plan.prepare(x, y)

            def eq():
                plan.launch(eq_args)

            def iirs():
                src = px
                for i in range(S):
                    dst = (py, pz)[i & 1]
                    gab.check(gab.lib.gab_iir(src, dst, iir_c, pst, T, B, stream))
                    src = dst

            for _ in range(20):
                eq()
                iirs()
            t_eq, t_iir = [], []
            rounds = 4
            for _ in range(rounds):                                  # alternated: both see the same clocks
                t_eq.append(events(eq, max(1, args.launches // rounds)))
                t_iir.append(events(iirs, max(1, args.launches // rounds)))
            t_eq, t_iir = float(np.median(t_eq)), float(np.median(t_iir))
            M, H = plan.form
            row = (29 + 2 * M + 3) // 4 * 4 * 4
            nbytes = 2 * T * B * 4 + T * S * (row + 16)
            print("%7d %3d %6s | %9.2f %9.2f %6.2f | %9.3g %8.3f" % (T, S, "%dx%d" % (M, H), t_eq, t_iir, t_iir / t_eq, nbytes,
                                                                    nbytes / (t_eq * 1e-6) / 8e12), flush=True)
            plan.close()


if __name__ == "__main__":
    main()
