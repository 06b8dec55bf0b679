"""Verified reconstruction of short stripes (hec_reconstruct_crc_rows_device*),
the part that needs no GPU: the symbols, the header, the argument checks that
return before the coder's device is looked at, the workspace size, and the
host-side planner under AddressSanitizer + UBSan
(tests/cpp/rows_planner_check.cpp, a stand-alone program with the sanitizer
runtime linked in; nothing is preloaded)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT, gpu_available

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_reconstruct_crc_rows_device", "hec_reconstruct_crc_rows_mixed_workspace_size",
         "hec_reconstruct_crc_rows_device_mixed")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
K, M, CELL, S = 6, 3, 512, 2
FULL = K * CELL


def uniform(handle, ctype=H.CHECKSUM_CRC32C, cell=CELL, stripes=S, bpc=512, data_len=0):
    """The uniform call with every buffer NULL but plausible sizes."""
    return H.lib.hec_reconstruct_crc_rows_device(handle, ctype, None, None, None, None, None, cell, stripes, bpc,
                                                 data_len, None, None, None, None)


def mixed(handle, ctype=H.CHECKSUM_CRC32C, cell=CELL, stripes=S, bpc=512, stripe_bytes=None):
    masks = (ctypes.c_uint64 * max(stripes, 1))(*([0x1FE] * max(stripes, 1)))
    lens = None if stripe_bytes is None else (ctypes.c_uint64 * len(stripe_bytes))(*stripe_bytes)
    return H.lib.hec_reconstruct_crc_rows_device_mixed(handle, ctype, None, None, None, None, masks, None, lens, cell,
                                                       stripes, bpc, None, None, None, None, 0, None)


@pytest.fixture()
def host_coder():
    c = H.Coder(K, M, H.HEC_DEVICE_HOST)
    yield c
    c.close()


def test_symbols_in_library_and_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in declared, name
        assert name in H.EXPORTS, name
    assert "data_len" in re.search(r"hec_reconstruct_crc_rows_device\s*\(([^;]*)\);", header).group(1)
    assert "stripe_bytes" in re.search(r"hec_reconstruct_crc_rows_device_mixed\s*\(([^;]*)\);", header).group(1)
    for name in ("reconstruct_crc_rows_device", "reconstruct_crc_rows_mixed_workspace_size",
                 "reconstruct_crc_rows_device_mixed"):
        assert hasattr(H.Coder, name), name
    assert callable(H.reconstruct_crc_rows_batch_mixed)


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5
    assert "#define HEC_ABI_VERSION 5" in open(HEADER).read()


def test_null_coder_is_invalid():
    assert uniform(None) == H.HEC_ERR_INVALID_ARG
    assert mixed(None) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_reconstruct_crc_rows_mixed_workspace_size(None, 16) == 0


def test_invalid_arguments_come_before_the_device(host_coder):
    """What needs neither a buffer nor a device is refused as an argument error
    even on a host-only coder: HEC_CHECKSUM_NULL and unknown types, cell_len or
    bytes_per_checksum of 0, data_len out of range, a stripe_bytes entry above
    k * cell_len."""
    h = host_coder.handle
    bad = H.HEC_ERR_INVALID_ARG
    for call in (uniform, mixed):
        assert call(h, ctype=H.CHECKSUM_NULL) == bad
        assert call(h, ctype=7) == bad
        assert call(h, cell=0) == bad
        assert call(h, bpc=0) == bad
    # data_len: in or before the last stripe but one, past the group, non-zero without stripes
    for stripes, data_len in ((S, (S - 1) * FULL), (S, 1), (S, S * FULL + 1), (0, 5)):
        assert uniform(h, stripes=stripes, data_len=data_len) == bad, (stripes, data_len)
    assert mixed(h, stripe_bytes=[FULL + 1, 0]) == bad
    assert mixed(h, stripe_bytes=[1, 2 ** 63]) == bad


def test_host_only_coder_is_refused_otherwise(host_coder):
    h = host_coder.handle
    dev = H.HEC_ERR_DEVICE
    assert uniform(h) == dev
    assert mixed(h) == dev
    for data_len in (0, S * FULL, (S - 1) * FULL + 1, S * FULL - 1):
        assert uniform(h, data_len=data_len) == dev, data_len
    assert uniform(h, stripes=0) == dev
    for lens in ([0, 0], [FULL, FULL], [1, FULL - 1], [CELL, CELL + 1]):
        assert mixed(h, stripe_bytes=lens) == dev, lens
    assert uniform(h, ctype=H.CHECKSUM_CRC32, bpc=100, cell=1000) == dev


@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (10, 4), (12, 6)])
def test_workspace_size(k, m):
    """Monotonic in stripes, never smaller than the full-stripe call's, and
    with room for a u32 and a u64 per stripe behind it."""
    c = H.Coder(k, m, H.HEC_DEVICE_HOST)
    try:
        counts = (0, 1, 2, 9, 37, 1024, 100000)
        sizes = [c.reconstruct_crc_rows_mixed_workspace_size(s) for s in counts]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        for s, size in zip(counts, sizes):
            assert size >= c.reconstruct_crc_mixed_workspace_size(s) + 12 * s, s
            assert size % 8 == 0
    finally:
        c.close()


@pytest.mark.skipif(gpu_available(), reason="CPU container only (a sanitized program never starts beside a GPU)")
def test_planner_under_address_and_ub_sanitizer():
    if not shutil.which(HIPCC):
        pytest.skip(f"needs hipcc ({HIPCC} is missing)")
    if not os.path.exists(os.path.join(PKG_DIR, "build", "ec_reconstruct_rows.o")):
        pytest.skip("needs the built kernel objects (build/ec_reconstruct_rows.o is missing)")
    target = "build/rows_planner_check"
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([os.path.join(PKG_DIR, target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 72 sampled batches and the one of all 1471 RS(10,4) loss patterns
    assert "rows_planner_check: ok, 73 batches" in r.stdout, r.stdout[-2000:]
