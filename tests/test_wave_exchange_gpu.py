"""The wave-held 1024-point transform's first exchange by lane-half swaps (the product library) against the same exchange
through LDS (the diagnostic build with GAB_WAVE_XCHG_LDS=1, loaded by path in a child process), bit for bit on every route
that runs the transform: tools/wave_exchange_check.py.  The swaps only move values — the same butterflies and twiddle
products run on the same values in the same operand order, in another lane — so the int32 views must be equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from plan_helpers import gab  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "wave_exchange_check.py")

ROUTES = ["split_T4_batch", "split_T4_per_buffer", "split_T4_engine",
          "split_T8_batch", "split_T8_per_buffer", "split_T8_engine",
          "classic_L1024_T2", "r2c_1024_T3"]


@pytest.fixture(scope="module")
def both(gab, tmp_path_factory):
    """(product outputs, LDS-form outputs): computed once, read by every test below."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("wave_exchange_check", TOOL)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert os.path.basename(gab._capi.LIB_PATH) == "libgab_hip.so"
    product = tool.routes(gab, torch)
    lib = os.path.join(ROOT, "gpuaudiobench_amd", "libgab_hip_ablate.so")
    assert os.path.exists(lib), "the diagnostic library is not built (GAB_BUILD_TAG=ablate GAB_ABLATE=1 python gpuaudiobench_amd/build.py)"
    path = str(tmp_path_factory.mktemp("wave_exchange") / "lds_form.npz")
    r = subprocess.run([sys.executable, TOOL, path], cwd=ROOT, env=dict(os.environ, GAB_LIB_PATH=lib, GAB_WAVE_XCHG_LDS="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    assert "libgab_hip_ablate.so, exchange 1 through LDS" in r.stdout, r.stdout
    with np.load(path) as z:
        lds_form = {k: z[k] for k in z.files}
    return product, lds_form


def test_the_check_covers_every_route(both):
    product, lds_form = both
    assert sorted(product) == sorted(ROUTES) == sorted(lds_form)


@pytest.mark.parametrize("route", ROUTES)
def test_swaps_give_the_bits_of_the_lds_exchange(both, route):
    product, lds_form = both
    a, b = product[route], lds_form[route]
    assert a.dtype == np.float32 and a.shape == b.shape and a.size > 0
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0.0          # a route that wrote nothing proves nothing
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "%s: %d of %d words differ" % (
        route, int((a.view(np.int32) != b.view(np.int32)).sum()), a.size)


def test_the_three_split_launch_forms_agree(both):
    """One batch launch, eleven per-buffer launches and the engine: the same eleven outputs."""
    product, _ = both
    for T in (4, 8):
        ref = product["split_T%d_batch" % T].view(np.int32)
        for form in ("per_buffer", "engine"):
            assert np.array_equal(product["split_T%d_%s" % (T, form)].view(np.int32), ref), (T, form)
