"""Verified reconstruction (hec_reconstruct_crc_device*), the part that needs
no GPU: the symbols, the header, and the argument checks that return before
anything touches a device."""
import ctypes
import json
import os
import re

import pytest

import hdfs_native_ec as H
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_reconstruct_crc_device", "hec_reconstruct_crc_mixed_workspace_size",
         "hec_reconstruct_crc_device_mixed")


def _null_call(handle, mixed):
    """Both calls with every buffer NULL but plausible sizes."""
    if mixed:
        masks = (ctypes.c_uint64 * 2)(0x1FE, 0x1FF)
        return H.lib.hec_reconstruct_crc_device_mixed(handle, H.CHECKSUM_CRC32C, None, None, None, None, masks, None,
                                                      512, 2, 512, None, None, None, None, 0, None)
    return H.lib.hec_reconstruct_crc_device(handle, H.CHECKSUM_CRC32C, None, None, None, None, None, 512, 2, 512,
                                            None, None, None, None)


def test_symbols_in_library_and_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in declared, name
        assert name in H.EXPORTS, name


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5


def test_host_only_coder_is_refused():
    c = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    try:
        assert _null_call(c.handle, False) == H.HEC_ERR_DEVICE
        assert _null_call(c.handle, True) == H.HEC_ERR_DEVICE
    finally:
        c.close()


def test_null_coder_is_invalid():
    assert _null_call(None, False) == H.HEC_ERR_INVALID_ARG
    assert _null_call(None, True) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_reconstruct_crc_mixed_workspace_size(None, 16) == 0


def _recorded_workspace_sizes():
    with open(os.path.join(ROOT, "tests", "golden", "mixed_workspace_sizes.json")) as f:
        table = json.load(f)
    return [(key, stripes, dict(zip(table["calls"], row)))
            for key, rows in table["sizes"].items() for stripes, row in zip(table["stripes"], rows)]


@pytest.mark.parametrize("key,stripes,recorded", _recorded_workspace_sizes(),
                         ids=[f"{key}-{stripes}" for key, stripes, _ in _recorded_workspace_sizes()])
def test_mixed_workspace_sizes_are_exact(key, stripes, recorded):
    """The four *_workspace_size calls against the values recorded from the
    library as it stood before the mixed calls shared one host-side planner
    (tests/golden/mixed_workspace_sizes.json; never regenerated from the code
    under test): a caller's allocation does not change by a byte."""
    codec, k, m = key.split("-")
    c = H.Coder(int(k), int(m), H.HEC_DEVICE_HOST, codec=codec)
    try:
        got = {"decode": c.decode_mixed_workspace_size(stripes),
               "reconstruct": c.reconstruct_mixed_workspace_size(stripes),
               "scrub": c.scrub_mixed_workspace_size(stripes),
               "reconstruct_crc": c.reconstruct_crc_mixed_workspace_size(stripes)}
    finally:
        c.close()
    assert got == recorded


def test_workspace_size_grows_with_stripes():
    c = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    try:
        sizes = [c.reconstruct_crc_mixed_workspace_size(s) for s in (1, 2, 9, 37, 1024, 100000)]
        assert sizes[0] > 0
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        # the plain mixed call's workspace plus one u32 per stripe for the lists
        for s, size in zip((1, 2, 9, 37, 1024, 100000), sizes):
            assert size >= c.reconstruct_mixed_workspace_size(s) + 4 * s
    finally:
        c.close()
