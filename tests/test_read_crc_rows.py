"""Verified striped read into a file-order buffer (hec_read_crc_rows_device*),
the part that needs no GPU: the symbols, the header, the order of the argument
checks on a host-only coder, the workspace size, and the host-side planner
under AddressSanitizer + UBSan (tests/cpp/read_rows_planner_check.cpp, a
stand-alone program with the sanitizer runtime linked in; nothing is
preloaded)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT, gpu_available

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_read_crc_rows_device", "hec_read_crc_rows_mixed_workspace_size", "hec_read_crc_rows_device_mixed")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
K, M, CELL, S = 6, 3, 512, 2
FULL = K * CELL
SENTINEL = 0x5A


class Buffers:
    """Host memory behind every pointer of a call, so that a call that got past
    its checks by mistake would show in it: nothing may be written."""

    def __init__(self):
        n = K + M
        self.file = (ctypes.c_uint8 * (S * FULL))(*([SENTINEL] * (S * FULL)))
        self.bad = (ctypes.c_uint8 * (S * n))()
        self.ws = (ctypes.c_uint8 * 4096)(*([SENTINEL] * 4096))

    def untouched(self):
        return (all(b == SENTINEL for b in self.file) and not any(self.bad) and all(b == SENTINEL for b in self.ws))


def uniform(handle, ctype=H.CHECKSUM_CRC32C, cell=CELL, stripes=S, bpc=512, data_len=0, file_stride=0, bufs=None):
    """The uniform call with NULL arrays but plausible sizes."""
    file_ptr = ctypes.addressof(bufs.file) if bufs else None
    bad_ptr = ctypes.addressof(bufs.bad) if bufs else None
    return H.lib.hec_read_crc_rows_device(handle, ctype, None, None, file_ptr, file_stride, cell, stripes, bpc,
                                          data_len, None, bad_ptr, None)


def mixed(handle, ctype=H.CHECKSUM_CRC32C, cell=CELL, stripes=S, bpc=512, stripe_bytes=None, file_stride=0, bufs=None,
          masks=0x1FE):
    masks = (ctypes.c_uint64 * max(stripes, 1))(*([masks] * max(stripes, 1)))
    lens = None if stripe_bytes is None else (ctypes.c_uint64 * len(stripe_bytes))(*stripe_bytes)
    file_ptr = ctypes.addressof(bufs.file) if bufs else None
    bad_ptr = ctypes.addressof(bufs.bad) if bufs else None
    ws_ptr = ctypes.addressof(bufs.ws) if bufs else None
    return H.lib.hec_read_crc_rows_device_mixed(handle, ctype, None, None, file_ptr, file_stride, masks, lens, cell,
                                                stripes, bpc, None, bad_ptr, ws_ptr, 4096 if bufs else 0, None)


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
    uniform_args = re.search(r"hec_read_crc_rows_device\s*\(([^;]*)\);", header).group(1)
    mixed_args = re.search(r"hec_read_crc_rows_device_mixed\s*\(([^;]*)\);", header).group(1)
    for word in ("d_file", "file_stride", "data_len", "d_expected", "d_bad"):
        assert word in uniform_args, word
    for word in ("d_file", "file_stride", "present", "stripe_bytes", "d_workspace"):
        assert word in mixed_args, word
    for name in ("read_crc_rows_device", "read_crc_rows_mixed_workspace_size", "read_crc_rows_device_mixed"):
        assert hasattr(H.Coder, name), name
    assert callable(H.read_crc_rows_batch)


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5
    assert "#define HEC_ABI_VERSION 5" in open(HEADER).read()


def test_mirrors_declare_the_calls():
    mirror = open(os.path.join(PKG_DIR, "csrc", "hdfs_ec.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "ec", "mi355x.rs")).read()
    for name in NAMES:
        assert name + "(" in mirror, name
        assert "fn " + name + "(" in rust, name
    for name in ("read_crc_rows_device", "read_crc_rows_mixed_workspace_size", "read_crc_rows_device_mixed"):
        assert re.search(r"\b" + name + r"\(", mirror), name
        assert re.search(r"pub (unsafe )?fn " + name + r"\(", rust), name


def test_null_coder_is_invalid():
    assert uniform(None) == H.HEC_ERR_INVALID_ARG
    assert mixed(None) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_read_crc_rows_mixed_workspace_size(None, 16) == 0


def test_invalid_arguments_come_before_the_device(host_coder):
    """What needs neither a buffer nor a device is refused as an argument error
    even on a host-only coder, with nothing written: HEC_CHECKSUM_NULL and
    unknown types, cell_len or bytes_per_checksum of 0, data_len out of range,
    a stripe_bytes entry above k * cell_len, a file_stride that is non-zero and
    below k * cell_len."""
    h = host_coder.handle
    bad = H.HEC_ERR_INVALID_ARG
    bufs = Buffers()
    for call in (uniform, mixed):
        assert call(h, ctype=H.CHECKSUM_NULL, bufs=bufs) == bad
        assert call(h, ctype=7, bufs=bufs) == bad
        assert call(h, cell=0, bufs=bufs) == bad
        assert call(h, bpc=0, bufs=bufs) == bad
        for stride in (1, 16, FULL - 16, FULL - 1):
            assert call(h, file_stride=stride, bufs=bufs) == bad, stride
    # data_len: in or before the last stripe but one, past the group, non-zero without stripes
    for stripes, data_len in ((S, (S - 1) * FULL), (S, 1), (S, S * FULL + 1), (0, 5)):
        assert uniform(h, stripes=stripes, data_len=data_len, bufs=bufs) == bad, (stripes, data_len)
    assert mixed(h, stripe_bytes=[FULL + 1, 0], bufs=bufs) == bad
    assert mixed(h, stripe_bytes=[1, 2 ** 63], bufs=bufs) == bad
    assert bufs.untouched()


def test_host_only_coder_is_refused_otherwise(host_coder):
    """Everything that passed the first group of checks is HEC_ERR_DEVICE on a
    host-only coder, whatever the buffers are (NULL arrays, no workspace, a
    mask with fewer than k units: those come behind it), and nothing is
    written."""
    h = host_coder.handle
    dev = H.HEC_ERR_DEVICE
    for bufs in (None, Buffers()):
        assert uniform(h, bufs=bufs) == dev
        assert mixed(h, bufs=bufs) == dev
        for data_len in (0, S * FULL, (S - 1) * FULL + 1, S * FULL - 1):
            assert uniform(h, data_len=data_len, bufs=bufs) == dev, data_len
        assert uniform(h, stripes=0, bufs=bufs) == dev
        assert mixed(h, stripes=0, bufs=bufs) == dev
        for lens in ([0, 0], [FULL, FULL], [1, FULL - 1], [CELL, CELL + 1]):
            assert mixed(h, stripe_bytes=lens, bufs=bufs) == dev, lens
        for stride in (FULL, FULL + 7, 4 * FULL):
            assert uniform(h, file_stride=stride, bufs=bufs) == dev
            assert mixed(h, file_stride=stride, bufs=bufs) == dev
        assert uniform(h, ctype=H.CHECKSUM_CRC32, bpc=100, cell=1000, bufs=bufs) == dev
        assert mixed(h, masks=0x3, bufs=bufs) == dev  # two units present: not looked at yet
        assert bufs is None or bufs.untouched()


@pytest.mark.parametrize("k,m", [(2, 1), (3, 2), (6, 3), (10, 4), (12, 6)])
def test_workspace_size(k, m):
    """Monotonic in stripes, 8-byte granular, with room for a u32 and a u64
    per stripe, and 0 for no coder."""
    c = H.Coder(k, m, H.HEC_DEVICE_HOST)
    try:
        counts = (0, 1, 2, 9, 37, 64, 65, 1024, 100000)
        sizes = [c.read_crc_rows_mixed_workspace_size(s) for s in counts]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        for s, size in zip(counts, sizes):
            assert size >= 12 * s, s
            assert size % 8 == 0
    finally:
        c.close()


@pytest.mark.skipif(gpu_available(), reason="CPU container only (a sanitized program never starts beside a GPU)")
def test_planner_under_address_and_ub_sanitizer():
    if not shutil.which(HIPCC):
        pytest.skip(f"needs hipcc ({HIPCC} is missing)")
    if not os.path.exists(os.path.join(PKG_DIR, "build", "ec_read_rows.o")):
        pytest.skip("needs the built kernel objects (build/ec_read_rows.o is missing)")
    target = "build/read_rows_planner_check"
    r = subprocess.run(["make", "-s", "-C", PKG_DIR, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([os.path.join(PKG_DIR, target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 96 sampled batches and the one of all 1471 RS(10,4) loss patterns
    assert "read_rows_planner_check: ok, 97 batches" in r.stdout, r.stdout[-2000:]
