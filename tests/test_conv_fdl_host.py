"""The fdl scheme of the conv plan (gab_conv_create_scheme) without a GPU: argument checks that come before any device
call, and the float64 whole-stream reference the GPU tests (test_conv_fdl_gpu.py) hold the scheme to."""
import ctypes as C

import numpy as np
import pytest

FDL = 2


def stream_reference(xs, ir, T, B, L):
    """Each channel's whole concatenated stream convolved with its response in float64 (scipy fftconvolve):
    xs = n buffers [T*B] (channel-major), ir [T*L]; returns n outputs [B*T] (sample-major, out[s*T + t]).
    ir may also be a schedule [(first_buffer, ir), ...] (the first entry at buffer 0): output buffer i then uses the
    response in force at i, over the whole input history (which does not depend on the taps)."""
    from scipy.signal import fftconvolve
    schedule = ir if isinstance(ir, (list, tuple)) else [(0, ir)]
    assert schedule[0][0] == 0 and all(a[0] < b[0] for a, b in zip(schedule, schedule[1:]))
    n = len(xs)
    X = np.stack([np.asarray(x, np.float64).reshape(T, B) for x in xs], axis=1).reshape(T, n * B)
    out = []
    for j, (first, h) in enumerate(schedule):
        end = schedule[j + 1][0] if j + 1 < len(schedule) else n
        if end <= first:
            continue
        H = np.asarray(h, np.float64).reshape(T, L)
        Y = np.stack([fftconvolve(X[t, :end * B], H[t])[:end * B] for t in range(T)])
        out += [np.ascontiguousarray(Y[:, i * B:(i + 1) * B].T).ravel() for i in range(first, end)]
    return out


@pytest.fixture(scope="module")
def lib():
    import gpuaudiobench_amd as g
    return g


@pytest.mark.parametrize("tracks,bufsize,ir_len,scheme", [
    (4, 300, 1000, FDL), (4, 64, 1000, FDL), (4, 4096, 1000, FDL), (4, 512, 0, FDL), (4, 512, 2 ** 21 + 1, FDL),
    (0, 512, 1000, FDL), (-3, 512, 1000, FDL), (4, 512, 1000, 3), (4, 512, 1000, -1)])
def test_create_scheme_refuses_bad_arguments_before_any_device_call(lib, tracks, bufsize, ir_len, scheme):
    # a device call on a machine without a GPU would fail with a runtime error, not GAB_ERR_INVALID_ARG
    h = C.c_void_p()
    rc = lib.lib.gab_conv_create_scheme(C.byref(h), tracks, bufsize, ir_len, scheme)
    assert rc == lib._capi.GAB_ERR_INVALID_ARG
    assert h.value is None
    text = lib.lib.gab_last_error().decode()
    assert "gab_conv_create_scheme" in text
    assert "GAB_CONV_SCHEME" not in text


def test_create_scheme_refuses_a_null_plan_pointer(lib):
    assert lib.lib.gab_conv_create_scheme(None, 4, 512, 1000, FDL) == lib._capi.GAB_ERR_INVALID_ARG
    assert "null" in lib.lib.gab_last_error().decode()


def test_create_scheme_classic_has_gab_conv_create_errors(lib):
    h = C.c_void_p()
    for scheme in (0, 1):
        assert lib.lib.gab_conv_create_scheme(C.byref(h), 0, 512, 1000, scheme) == lib._capi.GAB_ERR_INVALID_ARG
        assert lib.lib.gab_conv_create(C.byref(h), 0, 512, 1000) == lib._capi.GAB_ERR_INVALID_ARG
        assert h.value is None


def test_conv_plan_fdl_is_bound_in_python(lib):
    assert lib._capi.CONV_SCHEME_FDL == FDL
    assert "gab_conv_create_scheme" in lib._capi.PROTOTYPES
    names = [f[0] for f in lib._capi.BenchConfig._fields_]
    assert names[-1] == "conv_scheme"
    c = lib._capi.BenchConfig()
    c.conv_scheme = 5
    lib.lib.gab_bench_default_config(C.byref(c))
    assert c.conv_scheme == 0                                 # the default keeps gab_conv_create's routing


def test_stream_reference_equals_the_oracle_stream(orc):
    """The whole-stream float64 reference against the oracle's buffer-by-buffer float64 stream (which carries the
    history itself): T = 3, B = 128, L = 1000, 20 buffers."""
    T, B, L, n = 3, 128, 1000, 20
    rng = np.random.default_rng(7)
    ir = (rng.standard_normal((T, L)) * np.exp(-np.arange(L) / 250.0)).astype(np.float32).ravel()
    xs = [rng.standard_normal(T * B).astype(np.float32) for _ in range(n)]
    refs = stream_reference(xs, ir, T, B, L)
    hist = np.zeros(T * L, np.float32)
    peak = max(np.abs(r).max() for r in refs)
    for i in range(n):
        o = orc.conv_accel_stream(xs[i], ir, hist, L, B, T, f64=True)
        assert np.abs(o - refs[i]).max() <= 1e-12 * peak, i
