"""The argument builder of the verified calls (ec_capi.cpp: the survivors and
rows of a plan into the slots of a launch's argument block), checked on the
CPU against the filling restated from the plan alone, under AddressSanitizer +
UBSan (tests/cpp/launch_args_check.cpp, a stand-alone program with the
sanitizer runtime linked in; nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, gpu_available

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(gpu_available(), reason="CPU container only (a sanitized program never starts beside a GPU)")
def test_builder_under_address_and_ub_sanitizer():
    if not shutil.which(HIPCC):
        pytest.skip(f"needs hipcc ({HIPCC} is missing)")
    if not os.path.exists(os.path.join(PKG_DIR, "build", "ec_reconstruct_rows.o")):
        pytest.skip("needs the built kernel objects (build/ec_reconstruct_rows.o is missing)")
    target = "build/launch_args_check"
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([os.path.join(PKG_DIR, target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 4 codes x (n single losses + 24 x 2 seeded multiple losses + all parity lost) = 242 reconstruction plans, and
    # the check plan of every one of those masks that keeps more than k units
    assert "launch_args_check: ok, 368 plans, 2773 fills" in r.stdout, r.stdout[-2000:]
