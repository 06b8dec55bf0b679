"""Verified scrub (hec_scrub_crc_device*), the part that needs no GPU: the
symbols, the header, the bindings' names and the argument checks that can be
reached without a device.  A device coder cannot be created without a GPU, and
a host-only coder is refused before its other arguments are looked at, so the
HEC_ERR_INVALID_ARG cases that need a live coder are in test_gpu_scrub_crc.py
(test_invalid_arguments_queue_nothing)."""
import ctypes
import os
import re

import hdfs_native_ec as H
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_scrub_crc_device", "hec_scrub_crc_mixed_workspace_size", "hec_scrub_crc_device_mixed")


def _call(handle, mixed, ctype=None, stripes=2, cell=512, bpc=512, shards=None, strides=None, expected=None, bad=None,
          results=None, masks=None, ws=None, ws_bytes=0):
    """Either call; every buffer NULL unless given."""
    ctype = H.CHECKSUM_CRC32C if ctype is None else ctype
    if mixed:
        return H.lib.hec_scrub_crc_device_mixed(handle, ctype, shards, strides, masks, cell, stripes, bpc, expected,
                                                bad, results, ws, ws_bytes, None)
    return H.lib.hec_scrub_crc_device(handle, ctype, shards, strides, cell, stripes, bpc, expected, bad, results, None)


def test_symbols_in_library_and_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in declared, name
        assert name in H.EXPORTS, name


def test_header_says_what_can_be_captured():
    text = open(HEADER).read()
    at = text.index("Verified scrub:")
    comment = text[at:text.index("int hec_scrub_crc_device(", at)]
    assert "captured into a HIP graph" in comment
    assert "mixed form into a HIP graph is not supported" in comment
    assert "pays a launch each" in comment


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5
    assert "#define HEC_ABI_VERSION 5" in open(HEADER).read()


def test_python_names():
    for name in ("scrub_crc_device", "scrub_crc_mixed_workspace_size", "scrub_crc_device_mixed"):
        assert callable(getattr(H.Coder, name)), name
    assert callable(H.scrub_crc_batch) and callable(H.scrub_crc_batch_mixed)


def test_cpp_mirror_and_rust_names():
    mirror = open(os.path.join(ROOT, "hdfs-native_amd", "csrc", "hdfs_ec.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "ec", "mi355x.rs")).read()
    for name in ("scrub_crc_device", "scrub_crc_device_mixed", "scrub_crc_mixed_workspace_size"):
        assert re.search(r"\b%s\(" % name, mirror), name
        assert re.search(r"pub (unsafe )?fn %s\(" % name, rust), name
        assert re.search(r"\bfn hec_%s\(" % name, rust), name
        assert ("hec_%s(" % name) in mirror, name


def test_host_only_coder_is_refused():
    c = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    try:
        masks = (ctypes.c_uint64 * 2)(0x1FE, 0x1FF)
        assert _call(c.handle, False) == H.HEC_ERR_DEVICE
        assert _call(c.handle, True, masks=masks) == H.HEC_ERR_DEVICE
        # also with nothing to do and with no checksum type
        assert _call(c.handle, False, stripes=0) == H.HEC_ERR_DEVICE
        assert _call(c.handle, True, ctype=H.CHECKSUM_NULL, masks=masks) == H.HEC_ERR_DEVICE
    finally:
        c.close()


def test_null_coder_is_invalid():
    """With valid host stand-ins for every other argument, so that the NULL
    coder is what is refused; nothing is dereferenced."""
    n = 9
    buf = (ctypes.c_uint8 * 4096)()
    addr = ctypes.addressof(buf)
    shards, strides = H._pp([addr] * n), H._sp([512] * n)
    masks = (ctypes.c_uint64 * 2)(0x1FE, 0x1FF)
    for stripes in (0, 2):
        assert _call(None, False, stripes=stripes, shards=shards, strides=strides, expected=addr, bad=addr,
                     results=addr) == H.HEC_ERR_INVALID_ARG
        assert _call(None, True, stripes=stripes, shards=shards, strides=strides, expected=addr, bad=addr,
                     results=addr, masks=masks, ws=addr, ws_bytes=4096) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_scrub_crc_mixed_workspace_size(None, 16) == 0


def test_workspace_size_covers_the_lists_and_the_plain_call():
    for k, m, codec in ((6, 3, "rs"), (10, 4, "rs"), (3, 2, "rs"), (2, 1, "rs"), (5, 1, "xor"), (6, 6, "rs")):
        c = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
        try:
            counts = (0, 1, 2, 9, 17, 37, 1024, 100000)
            sizes = [c.scrub_crc_mixed_workspace_size(s) for s in counts]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
            for s, size in zip(counts, sizes):
                assert size >= 4 * s
                # the composed route runs the plain mixed call in the same workspace
                assert size >= c.scrub_mixed_workspace_size(s) + 4 * s
        finally:
            c.close()
