"""Composite CRCs (hec_crc_concat, hec_composite_crc), the part that needs no
GPU.  Ground truth is never the code under test: (a) the oracle's CRC over the
actual concatenated bytes, with chunk sums from the oracle; (b) the bit-at-a-
time restatement in composite_crc_ref.py, where the sums are opaque words."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import composite_crc_cases as cases
import composite_crc_ref as ref
import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
NAMES = ("hec_crc_concat", "hec_composite_crc", "hec_composite_crc_workspace_size", "hec_composite_crc_device")
TYPES = (H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32)
GUARD = 64


def test_symbols_in_header_library_and_bindings():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in declared, name
        assert name in H.EXPORTS, name
    assert callable(H.crc_concat) and callable(H.composite_crc) and callable(H.composite_crc_workspace_size)
    assert callable(H.Coder.composite_crc_device)
    mirror = open(os.path.join(PKG_DIR, "csrc", "hdfs_ec.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "ec", "mi355x.rs")).read()
    for name in NAMES:
        assert name + "(" in mirror, name
        assert re.search(r"\bfn %s\(" % name, rust), name


def test_abi_version_unchanged():
    assert H.lib.hec_abi_version() == 5
    assert "#define HEC_ABI_VERSION 5" in open(HEADER).read()


def test_catalogue_check_values(c_oracle):
    for ctype, check in ((H.CHECKSUM_CRC32C, 0xE3069283), (H.CHECKSUM_CRC32, 0x765E7680)):
        a = cases.oracle_crc(c_oracle, ctype, np.frombuffer(b"1234", dtype=np.uint8))
        b = cases.oracle_crc(c_oracle, ctype, np.frombuffer(b"56789", dtype=np.uint8))
        assert H.crc_concat(ctype, a, b, 5) == check
        assert ref.concat(ctype, a, b, 5) == check


def test_crc_empty_values(c_oracle):
    for ctype in TYPES:
        assert cases.oracle_crc(c_oracle, ctype, np.zeros(0, dtype=np.uint8)) == ref.crc_empty(ctype)


@pytest.mark.parametrize("ctype", TYPES)
def test_concat_against_oracle_bytes(c_oracle, ctype):
    rng = np.random.default_rng(20 + ctype)
    edge = (0, 1, 511, 512, 513)
    splits = list(itertools.product(edge, edge))
    splits += [(int(rng.integers(0, 3000)), int(rng.integers(0, 3000))) for _ in range(40)]
    for la, lb in splits:
        data = rng.integers(0, 256, la + lb, dtype=np.uint8)
        a = cases.oracle_crc(c_oracle, ctype, data[:la])
        b = cases.oracle_crc(c_oracle, ctype, data[la:])
        assert H.crc_concat(ctype, a, b, lb) == cases.oracle_crc(c_oracle, ctype, data), (la, lb)


@pytest.mark.parametrize("ctype", TYPES)
def test_concat_long_lengths_against_definition(ctype):
    rng = np.random.default_rng(30 + ctype)
    for len_b in (2**32 - 1, 2**32, 2**40 + 3, 2**63 - 1):
        for _ in range(4):
            a, b = int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))
            assert H.crc_concat(ctype, a, b, len_b) == ref.concat(ctype, a, b, len_b), len_b


def _host(ctype, sums, n, k, cell, stripes, bpc, data_len, want=(True, True, True)):
    """hec_composite_crc with each output inside 0xA5 guard bands; returns the
    three outputs as uint32 arrays (None where not asked for)."""
    sizes = (4 * stripes * n, 4 * n, 4)
    bufs = [(ctypes.c_uint8 * (size + 2 * GUARD))(*([0xA5] * (size + 2 * GUARD))) for size in sizes]
    ptrs = [ctypes.addressof(b) + GUARD if w else None for b, w in zip(bufs, want)]
    blob = np.ascontiguousarray(sums, dtype=np.uint8).tobytes()
    src = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
    rc = H.lib.hec_composite_crc(ctype, src, n, k, cell, stripes, bpc, data_len, *ptrs)
    assert rc == H.HEC_OK, rc
    assert bytes(src) == blob
    out = []
    for b, size, w in zip(bufs, sizes, want):
        raw = bytes(b)
        assert raw[:GUARD] == b"\xA5" * GUARD and raw[GUARD + size:] == b"\xA5" * GUARD
        if not w:
            assert raw == b"\xA5" * len(raw)  # a NULL output: nothing written anywhere
        out.append(cases.be_words(raw[GUARD:GUARD + size]) if w else None)
    return out


GEOMETRY = list(itertools.product(((9, 6), (14, 10), (5, 3), (1, 1)), (16, 37, 528, 1000, 9232), (256, 512, 4096),
                                  (1, 3, 40)))


def test_geometry_list_is_the_full_product():
    assert len(GEOMETRY) == 4 * 5 * 3 * 3


@pytest.mark.parametrize("ctype", TYPES)
def test_composite_against_oracle_bytes(c_oracle, ctype):
    """Every (n, k) x C x B x S; the data_len case rotates with the geometry,
    so each case meets every value of every other parameter."""
    for i, ((n, k), cell, bpc, stripes) in enumerate(GEOMETRY):
        data_len = cases.data_len_cases(k, cell, stripes)[(i + i // 5 + i // 25) % 5]
        sums, cells, units, group = cases.build(c_oracle, ctype, n, k, cell, stripes, bpc, data_len, seed=1000 + i)
        got = _host(ctype, sums, n, k, cell, stripes, bpc, data_len)
        where = (n, k, cell, bpc, stripes, data_len)
        assert np.array_equal(got[0], cells.reshape(-1)), where
        assert np.array_equal(got[1], units), where
        assert got[2][0] == group, where


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("n,k", ((9, 6), (14, 10), (5, 3), (1, 1)))
def test_every_data_len_case(c_oracle, ctype, n, k):
    for cell, bpc, stripes in ((37, 256, 3), (528, 512, 1), (1000, 256, 3)):
        for data_len in cases.data_len_cases(k, cell, stripes):
            sums, cells, units, group = cases.build(c_oracle, ctype, n, k, cell, stripes, bpc, data_len, seed=data_len)
            for want in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
                got = _host(ctype, sums, n, k, cell, stripes, bpc, data_len, want)
                assert got[0] is None or np.array_equal(got[0], cells.reshape(-1))
                assert got[1] is None or np.array_equal(got[1], units)
                assert got[2] is None or got[2][0] == group
            # the python wrapper
            py = H.composite_crc(ctype, sums.tobytes(), n, k, cell, stripes, bpc, data_len)
            assert py == (cells.tolist(), units.tolist(), group)


def opaque_sums(n, k, cell, stripes, bpc, data_len, seed, dead, parity_fill=None):
    """Random words as sums; the slots no chunk covers hold `dead`, and with
    parity_fill the whole of every parity unit's slots hold that byte."""
    rng = np.random.default_rng(seed)
    nck = -(-cell // bpc)
    sums = rng.integers(0, 256, (stripes, n, nck, 4), dtype=np.uint8)
    lens = ref.cell_lengths(n, k, cell, stripes, data_len)
    for u in range(n):
        sums[stripes - 1, u, -(-lens[stripes - 1][u] // bpc):] = dead
    if parity_fill is not None:
        sums[:, k:] = parity_fill
    return sums


def as_ints(sums):
    return sums.reshape(sums.shape[:3] + (4,)).view(">u4")[..., 0].astype(np.uint32).tolist()


OPAQUE = [  # n, k, cell, stripes, bpc, data_len
    (9, 6, 2**30, 8, 2**30, 0),                                # unit lengths past 2^32
    (9, 6, 2**30, 8, 2**30, 7 * 6 * 2**30 + 2**30 + 5),       # short last stripe, empty cells
    (5, 3, 1000, 3, 256, 2 * 3 * 1000 + 1000 + 300),
    (14, 10, 9232, 2, 512, 10 * 9232 + 3 * 9232),
]


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("geom", OPAQUE)
def test_composite_opaque_sums_against_definition(ctype, geom):
    n, k, cell, stripes, bpc, data_len = geom
    a = opaque_sums(n, k, cell, stripes, bpc, data_len, 7, 0xA5)
    b = opaque_sums(n, k, cell, stripes, bpc, data_len, 7, 0x5A)
    want_cells, want_units, want_group = ref.composite(ctype, as_ints(a), n, k, cell, stripes, bpc, data_len)
    got_a = _host(ctype, a, n, k, cell, stripes, bpc, data_len)
    got_b = _host(ctype, b, n, k, cell, stripes, bpc, data_len)
    assert got_a[0].reshape(stripes, n).tolist() == want_cells
    assert got_a[1].tolist() == want_units
    assert got_a[2][0] == want_group
    for x, y in zip(got_a, got_b):  # the dead slots have no effect
        assert np.array_equal(x, y)
    # nor have the parity slots on the group, the data units and the data cells
    pa = _host(ctype, opaque_sums(n, k, cell, stripes, bpc, data_len, 7, 0xA5, 0xA5), n, k, cell, stripes, bpc, data_len)
    pb = _host(ctype, opaque_sums(n, k, cell, stripes, bpc, data_len, 7, 0x5A, 0x5A), n, k, cell, stripes, bpc, data_len)
    assert pa[2][0] == pb[2][0] == want_group
    assert pa[1][:k].tolist() == pb[1][:k].tolist() == want_units[:k]
    assert np.array_equal(pa[0].reshape(stripes, n)[:, :k], pb[0].reshape(stripes, n)[:, :k])
    assert pa[0].reshape(stripes, n)[:, :k].tolist() == [row[:k] for row in want_cells]


def test_argument_errors():
    sums = (ctypes.c_uint8 * 4096)()
    out = (ctypes.c_uint8 * 4096)(*([0xA5] * 4096))
    ok = dict(ctype=H.CHECKSUM_CRC32C, sums=sums, n=9, k=6, cell=512, stripes=2, bpc=512, data_len=0)

    def call(**kw):
        a = dict(ok, **kw)
        return H.lib.hec_composite_crc(a["ctype"], a["sums"], a["n"], a["k"], a["cell"], a["stripes"], a["bpc"],
                                       a["data_len"], out, out, out)

    assert call() == H.HEC_OK
    out[:] = [0xA5] * 4096
    full = 2 * 6 * 512
    for bad in (dict(sums=None), dict(cell=0), dict(bpc=0), dict(n=0), dict(n=65), dict(k=0), dict(k=10),
                dict(data_len=full + 1), dict(data_len=full - 6 * 512), dict(data_len=1),
                dict(ctype=H.CHECKSUM_NULL), dict(ctype=3), dict(ctype=-1), dict(stripes=0, data_len=1)):
        assert call(**bad) == H.HEC_ERR_INVALID_ARG, bad
    assert call(data_len=full) == H.HEC_OK and call(data_len=full - 6 * 512 + 1) == H.HEC_OK
    assert call(n=64, k=64, cell=4, bpc=4, stripes=1) == H.HEC_OK
    out[:] = [0xA5] * 4096
    assert call(stripes=0) == H.HEC_OK  # nothing to do, nothing written
    assert bytes(out) == b"\xA5" * 4096
    word = ctypes.c_uint32()
    for ctype in (H.CHECKSUM_NULL, 3, -1):
        assert H.lib.hec_crc_concat(ctype, 1, 2, 3, ctypes.byref(word)) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_crc_concat(H.CHECKSUM_CRC32, 1, 2, 3, None) == H.HEC_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        H.crc_concat(H.CHECKSUM_NULL, 1, 2, 3)


def _device_call(handle, sums, ws, ws_bytes, stripes=2, ctype=H.CHECKSUM_CRC32C):
    return H.lib.hec_composite_crc_device(handle, ctype, sums, 9, 6, 512, stripes, 512, 0, sums, sums, sums, ws,
                                          ws_bytes, None)


def test_device_call_without_a_device():
    buf = (ctypes.c_uint8 * 4096)()
    c = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    try:
        assert _device_call(c.handle, buf, buf, 4096) == H.HEC_ERR_DEVICE
        assert _device_call(c.handle, buf, buf, 4096, stripes=0) == H.HEC_ERR_DEVICE
        with pytest.raises(H.DeviceError):
            c.composite_crc_device(H.CHECKSUM_CRC32C, ctypes.addressof(buf), 9, 6, 512, 2, 512)
    finally:
        c.close()
    for stripes in (0, 2):  # a NULL coder, every other argument valid
        assert _device_call(None, buf, buf, 4096, stripes=stripes) == H.HEC_ERR_INVALID_ARG


def test_workspace_size():
    assert H.composite_crc_workspace_size(0, 4) == 0 and H.composite_crc_workspace_size(65, 4) == 0
    for n in (1, 9, 14, 64):
        sizes = [H.composite_crc_workspace_size(n, s) for s in (0, 1, 2, 3, 64, 257, 4099, 65536)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] == 0 and sizes[1] == 4 * n
        assert all(size % 4 == 0 for size in sizes)
        # the cells' words plus at least one word per 1024 folded cells and fold
        assert sizes[-1] >= 4 * 65536 * n + 4 * (n + 1) * (65535 * n // 1024)


def test_standalone_sanitizer_check():
    """crc_compose.hpp's host part and the host entry point's body in one
    program under AddressSanitizer + UBSan (linked statically; plain where the
    runtime is not installed): exact-size heap buffers, the oracle as checker."""
    sources = [os.path.join(ROOT, "tests", "cpp", "composite_crc_check.cpp"),
               os.path.join(PKG_DIR, "csrc", "crc_compose.hpp"), os.path.join(PKG_DIR, "csrc", "checksum_tables.hpp")]
    binary = os.path.join(PKG_DIR, "build", "composite_crc_check")
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in sources):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, "build/composite_crc_check"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
