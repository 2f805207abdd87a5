#!/usr/bin/env python3
"""Device time of gab_iir in two builds of the library loaded into one process, alternating: this tree's libgab_hip.so and
a base build beside it (the sources of another commit in gpuaudiobench_amd/_csrc_<tag>/, built with
GAB_CSRC=... GAB_BUILD_TAG=<tag> python gpuaudiobench_amd/build.py).  HIP events around 20 back-to-back launches; a round's
figure is the median of 30 such samples; 9 rounds per library and shape, the order swapped every round.  Prints both sets,
the spread of the base's rounds, and whether this tree's median exceeds the base's by more than that spread.

    python tools/iir_ab.py [tag]        (default tag: parent)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpuaudiobench_amd")
BASE = sys.argv[1] if len(sys.argv) > 1 else "parent"
libs = {}
for tag, name in (("parent", "libgab_hip_%s.so" % BASE), ("this", "libgab_hip.so")):
    lib = C.CDLL(os.path.join(HERE, name))
    lib.gab_iir.restype = C.c_int
    lib.gab_iir.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    libs[tag] = lib
coeffs = (C.c_float * 5)(0.29287487, 0.58574975, 0.29287487, 5.120787e-08, 0.17149958)      # the reference's filter
ROUNDS, SAMPLES, PER = 9, 30, 20
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
for T, B in ((8192, 512), (65536, 512), (65536, 1024)):
    x = torch.rand(T * B, device="cuda") * 2 - 1
    y = torch.empty_like(x)
    st = {tag: torch.zeros(2 * T, device="cuda") for tag in libs}

    def launch(tag):
        rc = libs[tag].gab_iir(x.data_ptr(), y.data_ptr(), coeffs, st[tag].data_ptr(), T, B, stream)
        assert rc == 0, (tag, rc)

    outs = {}
    for tag in libs:                     # warm up, and the two agree on this input
        for _ in range(50):
            launch(tag)
        st[tag].zero_()
        launch(tag)
        outs[tag] = y.clone()
    torch.cuda.synchronize()
    diff = float((outs["parent"] - outs["this"]).abs().max() / outs["parent"].abs().max())
    meds = {tag: [] for tag in libs}
    for r in range(ROUNDS):
        for tag in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            samples = []
            for _ in range(SAMPLES):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(PER):
                    launch(tag)
                b.record()
                b.synchronize()
                samples.append(a.elapsed_time(b) * 1000.0 / PER)
            meds[tag].append(float(np.median(samples)))
    p, n = np.array(meds["parent"]), np.array(meds["this"])
    spread = float(p.max() - p.min())
    print("gab_iir %6d x %4d us/launch: parent median %.2f (rounds %s, spread %.2f) | this median %.2f (rounds %s) | "
          "this - parent %+.2f, within the parent's spread: %s | outputs differ by %.2g of peak"
          % (T, B, np.median(p), " ".join("%.2f" % v for v in p), spread, np.median(n), " ".join("%.2f" % v for v in n),
             np.median(n) - np.median(p), bool(np.median(n) - np.median(p) <= spread), diff))
    sys.stdout.flush()
