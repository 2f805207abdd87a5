"""The owners and the entry bodies of gab_plan.hpp under AddressSanitizer and UBSan, on the host alone.

tests/plan_owners/owners_main.cpp includes gab_plan.hpp with tests/plan_owners/hip/hip_runtime.h standing in for the
runtime (counting stubs, found first on the include path).  The program moves, re-allocates, swaps and half-builds
every owner and asserts that creates equal destroys and that no handle is destroyed twice; the sanitizers watch the
memory behind the handles.  tests/plan_owners/entries_main.cpp drives the bodies of the plans' extern "C" functions
(create_entry, entry, batch_entry, expose_entry) and the small helpers beside them with a fake plan: the texts, the
codes, the order of the checks, and that a refused or half-built create leaves null and nothing else behind.  Nothing
here touches a GPU or is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "plan_owners")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _run_under_sanitizers(tmp_path, source, ok):
    """Builds tests/plan_owners/<source> with the sanitizers and runs it; its output starts with `ok`."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    # (gcc: the runtimes inside the program, where clang puts them anyway)
    sanitize = SANITIZE + ([] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"])
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx] + sanitize + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip()[-200:])
    exe = tmp_path / "owners"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-self-move", "-Wno-unused-function"] + sanitize + [
        "-I" + HERE,                                          # hip/hip_runtime.h: the stand-in, ahead of any real one
        "-I" + os.path.join(ROOT, "gpuaudiobench_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(HERE, source), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith(ok), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_plan_owners_under_sanitizers(tmp_path):
    _run_under_sanitizers(tmp_path, "owners_main.cpp", "plan owners ok:")


def test_plan_entries_under_sanitizers(tmp_path):
    _run_under_sanitizers(tmp_path, "entries_main.cpp", "plan entries ok:")
