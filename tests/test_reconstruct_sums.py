"""Checksum-only reconstruction, the part that needs no GPU: the two calls
are in the library, the header and the binding, the ABI version did not move,
and they refuse a host-only or a NULL coder with a status."""
import ctypes
import os
import re

import hdfs_native_ec as H
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_reconstruct_sums_device", "hec_reconstruct_sums_device_mixed")


def test_symbols_in_library_header_and_exports():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", text))
    lib = ctypes.CDLL(H.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in declared, name
        assert name in H.EXPORTS, name


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5


def _args(n, S):
    """Host memory standing in for every buffer: neither call may get far
    enough to touch one."""
    cell = 512
    cells = (ctypes.c_uint8 * (S * n * cell))()
    base = ctypes.addressof(cells)
    ptrs = [base + i * cell for i in range(n)]
    sums = (ctypes.c_uint8 * (S * n * 4))()
    return cell, cells, ptrs, [n * cell] * n, sums


def test_host_only_coder_is_device_error():
    k, m, S = 6, 3, 2
    n = k + m
    cod = H.Coder(k, m, H.HEC_DEVICE_HOST)
    cell, cells, ptrs, strides, sums = _args(n, S)
    shards = [None] + ptrs[1:]
    rc = H.lib.hec_reconstruct_sums_device(cod.handle, H.CHECKSUM_CRC32C, H._pp([p or 0 for p in shards]),
                                           H._sp(strides), None, cell, S, 512, 0, None, None,
                                           ctypes.c_void_p(ctypes.addressof(sums)), None)
    assert rc == H.HEC_ERR_DEVICE
    masks = (ctypes.c_uint64 * S)(*([(1 << n) - 2] * S))
    ws = (ctypes.c_uint8 * 4096)()
    rc = H.lib.hec_reconstruct_sums_device_mixed(cod.handle, H.CHECKSUM_CRC32C, H._pp([p or 0 for p in shards]),
                                                 H._sp(strides), masks, None, cell, S, 512, None, None,
                                                 ctypes.c_void_p(ctypes.addressof(sums)),
                                                 ctypes.c_void_p(ctypes.addressof(ws)), 4096, None)
    assert rc == H.HEC_ERR_DEVICE
    assert not any(sums) and not any(cells)
    cod.close()


def test_null_coder_is_invalid_arg():
    n, S = 9, 2
    cell, cells, ptrs, strides, sums = _args(n, S)
    shards = [0] + ptrs[1:]
    rc = H.lib.hec_reconstruct_sums_device(None, H.CHECKSUM_CRC32C, H._pp(shards), H._sp(strides), None, cell, S,
                                           512, 0, None, None, ctypes.c_void_p(ctypes.addressof(sums)), None)
    assert rc == H.HEC_ERR_INVALID_ARG
    masks = (ctypes.c_uint64 * S)(*([(1 << n) - 2] * S))
    ws = (ctypes.c_uint8 * 4096)()
    rc = H.lib.hec_reconstruct_sums_device_mixed(None, H.CHECKSUM_CRC32C, H._pp(shards), H._sp(strides), masks, None,
                                                 cell, S, 512, None, None, ctypes.c_void_p(ctypes.addressof(sums)),
                                                 ctypes.c_void_p(ctypes.addressof(ws)), 4096, None)
    assert rc == H.HEC_ERR_INVALID_ARG
    assert not any(sums) and not any(cells)
