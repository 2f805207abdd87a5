"""Every route through the wave-held 1024-point transform (gab_fft.hpp, WaveFFT1024) on seeded inputs, outputs to one .npz:

    python tools/wave_exchange_check.py OUT.npz

Run once on the product library and once on the diagnostic build with the transform's first exchange through LDS
(GAB_LIB_PATH=gpuaudiobench_amd/libgab_hip_ablate.so GAB_WAVE_XCHG_LDS=1), the two files must hold the same bits:
tests/test_wave_exchange_gpu.py.  The lane-half swaps only move values, so nothing may differ.

Routes: the split cut (4096 taps, 512-sample buffers) on 4 channels (one workgroup) and on 8, eleven buffers — the history
ring of eight wraps and both far groups start on both parities — as one batch launch, as eleven per-buffer launches and
through the resident engine; the classic cut at 1024 taps on 2 channels; the 1024-point real-to-complex op on 3 tracks.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NBUF = 11


def routes(gab, torch):
    out = {}
    B, L = 512, 4096
    for T in (4, 8):
        n = T * B
        ir = torch.from_numpy(gab.harness.conv_accel_ir(L, T)).cuda()
        xs = [gab.harness.noise(n, seed=300 + 16 * T + k) for k in range(NBUF)]
        plan = gab.ConvPlan(T, B, L, scheme="split")
        plan.set_ir(ir)
        y = plan.process_batch(torch.from_numpy(np.concatenate(xs)).cuda(), NBUF)
        out["split_T%d_batch" % T] = y.cpu().numpy()
        plan.reset()
        ys = [plan.process(torch.from_numpy(x).cuda(), mode=gab.CONV_STREAMING).cpu().numpy() for x in xs]
        out["split_T%d_per_buffer" % T] = np.concatenate(ys)
        plan.reset()
        h_in, h_out = torch.empty(n).pin_memory(), torch.empty(n).pin_memory()
        plan.engine_start(4, stream=torch.cuda.Stream())
        ys = []
        for x in xs:
            h_in.copy_(torch.from_numpy(x))
            plan.engine_round_trip(h_in, h_out)
            ys.append(h_out.numpy().copy())
        plan.engine_stop()
        out["split_T%d_engine" % T] = np.concatenate(ys)
        plan.close()
    T, L = 2, 1024
    plan = gab.ConvPlan(T, B, L, scheme="classic")
    plan.set_ir(torch.from_numpy(gab.harness.conv_accel_ir(L, T)).cuda())
    ys = [plan.process(torch.from_numpy(gab.harness.noise(T * B, seed=500 + k)).cuda(), mode=gab.CONV_STREAMING).cpu().numpy()
          for k in range(4)]
    out["classic_L1024_T2"] = np.concatenate(ys)
    plan.close()
    x = torch.from_numpy(gab.harness.noise(3 * 1024, seed=77)).cuda()
    out["r2c_1024_T3"] = gab.fft_r2c_1024(x, 3).cpu().numpy()
    return out


if __name__ == "__main__":
    import torch
    import gpuaudiobench_amd as gab
    np.savez(sys.argv[1], **routes(gab, torch))
    print("wave_exchange_check: %s, exchange 1 %s" % (
        os.path.basename(gab._capi.LIB_PATH), "through LDS" if os.environ.get("GAB_WAVE_XCHG_LDS") else "by lane-half swaps"))
