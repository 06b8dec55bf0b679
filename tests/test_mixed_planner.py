"""The host-side planner of the per-stripe ("mixed") device calls, on the CPU,
under sanitizers: tests/cpp/planner_check.cpp includes csrc/ec_capi.cpp, plans
batches on host-only coders and compares every workspace image, byte for byte
and written into a heap buffer of exactly the planned size, with a reference
of its own (oracle matrix routines).  Built twice by the Makefile: with
AddressSanitizer + UBSan (every shape, planner and stripe count) and with
ThreadSanitizer (four threads on two shared coders).  Both are stand-alone
executables with the sanitizer runtime linked in; nothing is preloaded.

Never started where a GPU is visible; skipped only where hipcc or the built
kernel objects are missing.  A missing sanitizer runtime fails the build and
with it the test: there is no plain fallback."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, gpu_available

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL_OBJECTS = ("ec_kernels", "ec_reconstruct", "ec_reconstruct_crc", "ec_scrub", "ec_scrub_mixed", "ec_scrub_crc",
                  "ec_fused", "checksum", "tuning", "host_gf", "jit")

pytestmark = pytest.mark.skipif(gpu_available(), reason="CPU container only (a sanitized program never starts beside a GPU)")


def _build(target):
    if not shutil.which(HIPCC):
        pytest.skip(f"needs hipcc ({HIPCC} is missing)")
    missing = [n for n in KERNEL_OBJECTS if not os.path.exists(os.path.join(PKG_DIR, "build", n + ".o"))]
    if missing:
        pytest.skip("needs the built kernel objects (missing: " + ", ".join(f"build/{n}.o" for n in missing) + ")")
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(PKG_DIR, target)


def test_planner_under_address_and_ub_sanitizer():
    binary = _build("build/planner_check")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "planner_check: ALL OK shapes=13 " in r.stdout, r.stdout[-2000:]


def test_planner_threads_under_thread_sanitizer():
    binary = _build("build/planner_check_tsan")
    r = subprocess.run([binary, "threads"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "planner_check: ALL OK threads=4 " in r.stdout, r.stdout[-2000:]
