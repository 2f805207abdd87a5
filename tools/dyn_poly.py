#!/usr/bin/env python3
"""The two polynomials of the dynamics plan (include/gab_c_api.h, gab_dyn_*), fitted on the host in float64.

    log2(1 + t) = t r(t),  r of degree 6, t in [0, 1)       coefficients c0..c6
    exp2(f)     = q(f),    q of degree 6, f in [0, 1)       coefficients d0..d6, d0 = 1 exactly

Each is an interpolation at Chebyshev nodes (numpy only), no Remez pass: r interpolates log2(1 + t) / t at seven
nodes, and q = 1 + f p(f) with p interpolating (exp2(f) - 1) / f at six, which pins d0.  Every coefficient is rounded
to float32 once.  The script prints them as hex floats, the way k_dynamics.hip pins them, and measures both with the
float32 Horner chain of the contract (fmaf by fmaf; the fmaf here is a float64 product and sum rounded to float32,
which differs from a true fmaf only in rare double roundings: tests/test_dynamics_host.py holds the bounds with an
exact one).

    python tools/dyn_poly.py            prints the coefficients and the measured errors
    python tools/dyn_poly.py --check    also compares them with the library's pinned ones (gab_dyn_poly)
"""
import sys

import numpy as np

DEGREE = 6


def cheb_nodes(n):
    k = np.arange(n, dtype=np.float64)
    return 0.5 + 0.5 * np.cos((2.0 * k + 1.0) * np.pi / (2.0 * n))       # on [0, 1]


def interpolate(fn, n):
    """Ascending monomial coefficients (float64) of the degree n - 1 interpolant of fn at n Chebyshev nodes."""
    x = cheb_nodes(n)
    return np.linalg.solve(np.vander(x, n, increasing=True), fn(x))      # 7 x 7 at most: well within float64


def log2_coeffs():
    return interpolate(lambda t: np.log2(1.0 + t) / t, DEGREE + 1).astype(np.float32)


def exp2_coeffs():
    p = interpolate(lambda f: (np.exp2(f) - 1.0) / f, DEGREE)
    return np.concatenate([[1.0], p]).astype(np.float32)


def horner32(c, x):
    r = np.full(x.shape, c[-1], np.float32)
    for k in range(len(c) - 2, -1, -1):
        r = (r.astype(np.float64) * x.astype(np.float64) + np.float64(c[k])).astype(np.float32)
    return r


def measure(c, d, chunk=1 << 21):
    worst_log = worst_exp = 0.0
    for lo in range(0, 1 << 23, chunk):
        m = (np.arange(lo, lo + chunk, dtype=np.uint32) | np.uint32(0x3f800000)).view(np.float32)
        t = m - np.float32(1.0)
        L = t * horner32(c, t)
        worst_log = max(worst_log, float(np.abs(L.astype(np.float64) - np.log2(m.astype(np.float64))).max()))
    f = (np.arange(1 << 21, dtype=np.float64) / float(1 << 21)).astype(np.float32)
    q = horner32(d, f).astype(np.float64)
    worst_exp = float(np.abs(q / np.exp2(f.astype(np.float64)) - 1.0).max())
    return worst_log, worst_exp


def main():
    c, d = log2_coeffs(), exp2_coeffs()
    for name, v in (("log2 c", c), ("exp2 d", d)):
        for k, x in enumerate(v):
            mant, exp = float(x).hex().split("p")
            mant = mant.rstrip("0")
            print("%s%d = %-18s  %.9g" % (name, k, mant + ("0" if mant.endswith(".") else "") + "p" + exp + "f", x))
    wl, we = measure(c, d)
    print("log2: worst absolute error over 2^23 mantissas %.3g (2^%.2f), bound 2^-18" % (wl, np.log2(wl)))
    print("exp2: worst relative error over 2^21 points    %.3g (2^%.2f), bound 2^-22" % (we, np.log2(we)))
    ok = wl <= 2.0 ** -18 and we <= 2.0 ** -22 and d[0] == 1.0
    if "--check" in sys.argv:
        import ctypes as C
        import os
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from gpuaudiobench_amd import _capi
        pc, pd, nc, nd = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int(0), C.c_int(0)
        _capi.check(_capi.lib.gab_dyn_poly(C.byref(pc), C.byref(nc), C.byref(pd), C.byref(nd)))
        same = (nc.value == len(c) and nd.value == len(d) and all(pc[k] == c[k] for k in range(len(c)))
                and all(pd[k] == d[k] for k in range(len(d))))
        print("the library pins these coefficients:", same)
        ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
