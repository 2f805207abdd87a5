"""The conv plan's routes per channel at unequal levels (the "channel pairs" paragraph of include/gab_c_api.h): for each
route of tests/test_conv_levels_gpu.py, on that test's own streams,

    c_twin   the float32 packed-pair restatement of the route's cut against float64 (tests/conv_pair_twin.py)
    c_gpu    the plan against float64, the same figure: max |y_t - truth_t| / (peak_t + peak_p) over the channels
    ratio    c_gpu / c_twin (the tests gate it at 4)
    silent   what a silent channel beside a loud partner gives, in dB of the partner's peak (the plan, the restatement)
    nan      buffers a NaN at one sample of channel 0 kept its pair away from the clean stream's bits (the struck
             buffer included), beside tests/conv_pair_twin.nan_stay's figure for the route
    one-hot, impulse   the largest c_gpu / c_twin of the known answers: one-hot responses at the partition edges
             (the delayed input), a unit impulse (the response itself)

and the same three figures of gab_fft_r2c_1024 per track count.  Everything is a device result compared on the host:
no timing.

    python tools/conv_levels.py [--out FILE]      (profiles/r18_conv_levels.txt: this table, with notes added by hand)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def db(x):
    return "%7.1f" % (20 * np.log10(x)) if x > 0 else "  zeros"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import gpuaudiobench_amd as gab
    import conv_pair_twin as tw
    from test_conv_fdl_host import stream_reference
    from test_conv_plan_state_gpu import ROUTES, fill_len

    def stream(route, ir, xs):
        T, B, L, arg, _, _ = ROUTES[route]
        p = gab.ConvPlan(T, B, L, scheme=arg)
        p.set_ir(torch.from_numpy(ir).cuda())
        ys = [p.process(torch.from_numpy(x).cuda()).cpu().numpy() for x in xs]
        p.close()
        return ys

    lines = ["# tools/conv_levels.py on an MI355X: per-channel figures of the conv routes at unequal levels",
             "# levels 1, 2^-10 | 1, 0 | 2^-20, 2^-20 | 1, 1 (cut to T); c = max |y - float64| / (peak_t + peak_partner), window full",
             "# silent: levels 1, 0 | 0, 0 | 1, 1 | 0, 0; a silent pair gave zeros on every route (asserted)",
             "%-13s %2s %5s %6s %9s %9s %6s %13s %14s %11s %7s %7s" % (
                 "route", "T", "B", "L", "c_twin", "c_gpu", "ratio", "silent dB gpu", "silent dB twin", "nan gpu/fig",
                 "one-hot", "impulse")]
    for route in tw.LEVEL_ROUTES:
        T, B, L, _, _, kind = ROUTES[route]
        paired, first = kind in tw.PAIRED, fill_len(B, L)
        ir, xs = tw.levels_case(T, B, L, kind)
        truth = stream_reference(xs, ir, T, B, L)
        ct, _ = tw.channel_figures(tw.twin_stream(kind, xs, ir, T, B, L), truth, T, B, first, paired)
        cg, _ = tw.channel_figures(stream(route, ir, xs), truth, T, B, first, paired)
        # silence
        lv = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0])[:T]
        ir_s, xs_s = tw.levels_case(T, B, L, kind, lv, seed=3)
        peak = np.abs(tw.per_channel(stream_reference(xs_s, ir_s, T, B, L), T, B)).max(axis=(1, 2))
        ys = tw.per_channel(stream(route, ir_s, xs_s), T, B)
        yt = tw.per_channel(tw.twin_stream(kind, xs_s, ir_s, T, B, L), T, B)
        assert not ys[2:4].any(), route
        s_gpu, s_twin = np.abs(ys[1]).max() / peak[0], np.abs(yt[1]).max() / peak[0]
        # a NaN
        i = first + 1
        stay = tw.nan_stay(kind, B, L)
        xn = tw.noise(T, B, i + stay + 4, 8, tw.levels(T))
        xd = [x.copy() for x in xn]
        xd[i][B // 3] = np.nan
        clean, dirty = tw.per_channel(stream(route, ir, xn), T, B), tw.per_channel(stream(route, ir, xd), T, B)
        own = [0] if kind == "direct" else [t for t in (0, 1) if t < T]
        differs = [k for k in range(len(xn)) if not np.array_equal(clean[own, k].view(np.uint32), dirty[own, k].view(np.uint32))]
        rest = [t for t in range(T) if t not in own]
        assert np.array_equal(clean[rest].view(np.uint32), dirty[rest].view(np.uint32)), route
        # known answers
        def ratio(ir_k, xs_k, want):
            a, _ = tw.channel_figures(tw.twin_stream(kind, xs_k, ir_k, T, B, L), want, T, B, 0, paired)
            b, _ = tw.channel_figures(stream(route, ir_k, xs_k), want, T, B, 0, paired)
            return tw.c_max(b) / tw.c_max(a) if tw.c_max(a) > 0 else (0.0 if tw.c_max(b) == 0 else np.inf)
        n = tw.stream_len(T, B, L, kind)
        xk = tw.noise(T, B, n, 9)
        hot = max(ratio(ir_k, xk, tw.delayed(xk, taps, T, B)) for taps, ir_k in tw.one_hot_cases(T, B, L, kind))
        ir_i = tw.decaying_ir(T, L, B, 10)
        xi = [np.zeros(T * B, np.float32) for _ in range(n)]
        xi[0].reshape(T, B)[:, 0] = 1.0
        imp = ratio(ir_i, xi, stream_reference(xi, ir_i, T, B, L))
        lines.append("%-13s %2d %5d %6d %9.3g %9.3g %6.2f %13s %14s %7d/%-3d %7.3f %7.3f" % (
            route, T, B, L, tw.c_max(ct), tw.c_max(cg), tw.c_max(cg) / tw.c_max(ct), db(s_gpu), db(s_twin),
            differs[-1] - i + 1, stay, hot, imp))
    lines += ["", "# gab_fft_r2c_1024: c = max over bins |X_t - rfft64| / (spectral peak_t + peak_partner), the same levels",
              "# known: impulses at 0, 1, 511, 512, 1023, DC, alternating, cosines on bins 1, 255, 256, 511 (every peak 1): c_gpu / c_twin",
              "%-13s %2s %9s %9s %6s %13s %7s" % ("fft", "T", "c_twin", "c_gpu", "ratio", "silent dB gpu", "known")]
    for T in (1, 2, 3, 9, 17):
        rng = np.random.default_rng(100 + T)
        x = (rng.standard_normal((T, 1024)) * tw.levels(T)[:, None]).astype(np.float32).ravel()
        truth = tw.fft_truth(x, T)
        ct, _ = tw.fft_figures(tw.fft_pair_twin(x, T), truth)
        X = gab.fft_r2c_1024(torch.from_numpy(x).cuda(), T).cpu().numpy().astype(np.float64)
        X = X[..., 0] + 1j * X[..., 1]
        cg, _ = tw.fft_figures(X, truth)
        silent = db(np.abs(X[3]).max() / np.abs(truth[2]).max()) if T > 3 else "      -"
        xk, _ = tw.fft_known_answers(T)
        xk = xk.astype(np.float32).ravel()
        tk = tw.fft_truth(xk, T)
        Xk = gab.fft_r2c_1024(torch.from_numpy(xk).cuda(), T).cpu().numpy().astype(np.float64)
        known = tw.c_max(tw.fft_figures(Xk[..., 0] + 1j * Xk[..., 1], tk)[0]) / tw.c_max(tw.fft_figures(tw.fft_pair_twin(xk, T), tk)[0])
        lines.append("%-13s %2d %9.3g %9.3g %6.2f %13s %7.3f" % ("r2c_1024", T, tw.c_max(ct), tw.c_max(cg), tw.c_max(cg) / tw.c_max(ct), silent, known))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
