"""The C-ABI library loads and exports every symbol include/gab_c_api.h declares
(no compute calls: this runs without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gab_c_api.h")
LIB = os.path.join(ROOT, "gpuaudiobench_amd", "libgab_hip.so")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b(gab_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for must in ("gab_gain", "gab_conv_process", "gab_fdtd_process", "gab_bench_create",
                 "gab_fft_r2c_1024", "gab_rndmem", "gab_dwg", "gab_iir", "gab_modal",
                 "gab_datatransfer", "gab_gainstats", "gab_noop", "gab_conv1d",
                 "gab_debug_fdtd_form", "gab_debug_dwg_route", "gab_debug_modal_launch"):
        assert must in names
    assert len(names) >= 40


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build it with: python gpuaudiobench_amd/build.py"
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing


def test_python_binding_table_matches_header():
    from gpuaudiobench_amd import _capi
    assert sorted(_capi.PROTOTYPES) == declared_functions()


def test_version_and_errors_without_gpu():
    from gpuaudiobench_amd import _capi
    assert _capi.lib.gab_version() == 100
    # argument validation happens before any device call
    assert _capi.lib.gab_gainstats(None, None, None, 0, 0, 0.5, None) == _capi.GAB_ERR_INVALID_ARG
    assert b"null pointer" in _capi.lib.gab_last_error()
    h = ctypes.c_void_p()
    assert _capi.lib.gab_conv_create(ctypes.byref(h), -1, 512, 512) == _capi.GAB_ERR_INVALID_ARG
    assert _capi.lib.gab_bench_create(ctypes.byref(h), b"NoSuchBenchmark", None) == _capi.GAB_ERR_INVALID_ARG


def test_product_package_does_not_touch_the_oracle():
    """The product may not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "gpuaudiobench_amd")
    for dirpath, _, files in os.walk(pkg):
        if "_build" in dirpath or "__pycache__" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in text and "from oracle" not in text, f
                assert "gab_oracle" not in text and "orc_" not in text, f
    out = os.popen("ldd %s" % LIB).read()
    assert "oracle" not in out


def test_plans_refuse_the_runtime_mode_that_hung():
    """AMD_DIRECT_DISPATCH=0 hung a process in round 1 (cause unknown): plans refuse it with a clear
    error before any device call — checked in a child process, without a GPU."""
    import subprocess, sys, os
    code = ("import ctypes as C, gpuaudiobench_amd as g\n"
            "h = C.c_void_p()\n"
            "rc = g.lib.gab_conv_create(C.byref(h), 4, 512, 512)\n"
            "print(rc, g.lib.gab_last_error().decode())\n")
    env = dict(os.environ, AMD_DIRECT_DISPATCH="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    rc, text = r.stdout.strip().split(" ", 1)
    assert int(rc) == -3 and "AMD_DIRECT_DISPATCH" in text


def test_product_library_has_no_work_skipping_switches():
    """Stage ablations, stamps and kernel-form overrides (GAB_CONV_SPLIT_DEBUG, GAB_FDTD_*, ...) exist
    only in diagnostic builds (-DGAB_ABLATE -> libgab_hip_ablate.so): the product library and the
    driver do not contain the names, so no environment variable can make a product kernel skip work."""
    blob = open(LIB, "rb").read()
    driver = os.path.join(ROOT, "gpuaudiobench_amd", "gpubench")
    if os.path.exists(driver):
        blob += open(driver, "rb").read()
    # the three form queries of the header are product symbols: host functions that report what a launcher would do and
    # make no device call.  Every other gab_debug_ entry stays a diagnostic build's.
    for query in (b"gab_debug_fdtd_form", b"gab_debug_dwg_route", b"gab_debug_modal_launch"):
        assert query in blob, query
        blob = blob.replace(query, b"")
    for name in (b"GAB_CONV_SPLIT_DEBUG", b"GAB_CONV_STAMP_AT", b"GAB_CONV_RANGE_THREADS", b"GAB_CONV_ABLATE",
                 b"GAB_CONV_SCHEME", b"GAB_FDTD_GRAPH", b"GAB_FDTD_LDS", b"GAB_FDTD_TILE", b"GAB_FDTD_STAGGER",
                 b"g_split_stamps", b"gab_debug_"):
        assert name not in blob, name
    # the only environment variable the product reads is the runtime mode it refuses
    import re
    src_dir = os.path.join(ROOT, "gpuaudiobench_amd", "csrc")
    for f in sorted(os.listdir(src_dir)):
        text = open(os.path.join(src_dir, f), errors="replace").read()
        text = re.sub(r"#ifdef GAB_ABLATE.*?#endif", "", text, flags=re.S)
        for var in re.findall(r'getenv\("([A-Z_0-9]+)"\)', text):
            assert var == "AMD_DIRECT_DISPATCH", (f, var)
