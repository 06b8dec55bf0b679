"""Scrub correction on the CPU (hec_scrub_correct): scrub a stripe and fix the
one located unit in place.  Expected values come from scrub_correct_ref.py, a
numpy restatement of the definition (the verdict from the reference pair, then
e = scale * s_row applied to the named unit) over the oracle's matrix and
product table; every comparison is exact, and where exactly one unit was
corrupted the stripe is also compared with the untouched truth.  Then the C++
mirror and the host routine's sanitizer driver."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
import scrub_correct_ref as R
from conftest import PKG_DIR, ROOT

CODECS = [("rs", 3, 2), ("rs", 6, 3), ("rs", 10, 4), ("xor", 5, 1), ("rs-legacy", 6, 3)]  # tests/test_scrub.py's
BLOCK = 65536  # the host routine's block: 65536 + 17 crosses it
LENS = (1, 15, 16, 17, 64, 4099, BLOCK + 17)

_STRIPES = {}


def _stripe(codec, k, m):
    """A consistent stripe at the longest length (computed once); a shorter
    stripe is a prefix of every unit."""
    key = (codec, k, m)
    if key not in _STRIPES:
        rng = np.random.default_rng(9000 + 100 * k + m + len(codec))
        data = [rng.integers(0, 256, size=max(LENS), dtype=np.uint8) for _ in range(k)]
        _STRIPES[key] = data + O.matmul_shards(O.codec_matrix(codec, k, m)[k:], data)
    return _STRIPES[key]


def _copies(codec, k, m, length):
    return [np.ascontiguousarray(u[:length]).copy() for u in _stripe(codec, k, m)]


def _correct_raw(coder, units, with_out=True):
    """hec_scrub_correct on the given arrays, in place; -> (status, ruled_out, bad_bytes, unit)."""
    res = (ctypes.c_uint64 * 2)(0xDEAD, 0xBEEF)
    unit = ctypes.c_int(77)
    rc = coder._lib.hec_scrub_correct(coder.handle, H._pp([u.ctypes.data for u in units]), len(units[0]),
                                      res if with_out else None, ctypes.byref(unit))
    return rc, int(res[0]), int(res[1]), unit.value


@pytest.fixture(scope="module", params=CODECS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def case(request):
    codec, k, m = request.param
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    yield codec, k, m, coder
    coder.close()


def test_constants_and_abi():
    assert (H.CORRECT_CLEAN, H.CORRECT_UNLOCATED) == (-1, -2) == (R.CLEAN, R.UNLOCATED)
    assert H.lib.hec_abi_version() == 5


def test_every_unit_three_ways(case):
    """Unit t corrupt at byte 0, at the last byte, and as a whole: corrected
    bit-exactly (m >= 2), unit == t, the pair is the corrupted stripe's."""
    codec, k, m, coder = case
    rng = np.random.default_rng(17)
    for length in LENS:
        truth = _copies(codec, k, m, length)
        for t in range(k + m):
            for how in ("first", "last", "random"):
                units = [u.copy() for u in truth]
                if how == "first":
                    units[t][0] ^= 1 << (t % 8)
                elif how == "last":
                    units[t][length - 1] ^= 0x80 >> (t % 8)
                else:
                    units[t][:] = rng.integers(0, 256, size=length, dtype=np.uint8)
                    if np.array_equal(units[t], truth[t]):
                        units[t][0] ^= 1
                ruled, bad, unit, want = R.correct_stripe(codec, k, m, units)
                assert unit == (t if m > 1 else R.UNLOCATED), (codec, length, t, how)
                got = _correct_raw(coder, units)
                assert got == (H.HEC_OK, ruled, bad, unit), (codec, length, t, how)
                assert np.array_equal(np.stack(units), want), (codec, length, t, how)
                if m > 1:
                    assert np.array_equal(np.stack(units), np.stack(truth)), (codec, length, t, how)


def test_clean_stripe_is_untouched(case):
    codec, k, m, coder = case
    for length in LENS:
        truth = _copies(codec, k, m, length)
        units = [u.copy() for u in truth]
        assert _correct_raw(coder, units) == (H.HEC_OK, 0, 0, H.CORRECT_CLEAN), length
        assert np.array_equal(np.stack(units), np.stack(truth))
        assert R.correct_stripe(codec, k, m, units)[:3] == (0, 0, R.CLEAN)


def test_two_corrupt_units(case):
    """Two corrupt units at one position: -2 and untouched for m >= 3 and for
    m == 1; for m == 2 whatever the definition gives (LOCATED assumes at most
    one corrupt unit), which the restatement computes."""
    codec, k, m, coder = case
    n = k + m
    rng = np.random.default_rng(23)
    for length in LENS:
        for a, b in ((0, 1), (k - 1, k), (k, n - 1), (0, n - 1)):
            if a == b:
                continue
            units = _copies(codec, k, m, length)
            ea, eb = (int(v) for v in rng.integers(1, 256, size=2))
            units[a][length // 2] ^= ea
            units[b][length // 2] ^= eb
            before = np.stack(units)
            ruled, bad, unit, want = R.correct_stripe(codec, k, m, units)
            if m != 2:
                assert unit == R.UNLOCATED and np.array_equal(want, before)
            assert _correct_raw(coder, units) == (H.HEC_OK, ruled, bad, unit), (codec, length, a, b)
            assert np.array_equal(np.stack(units), want), (codec, length, a, b)


def test_two_units_two_positions_m2_is_multiple():
    codec, k, m = "rs", 3, 2
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    units = _copies(codec, k, m, 4099)
    units[1][0] ^= 0x40
    units[4][4098] ^= 0x02
    before = np.stack(units)
    assert _correct_raw(coder, units) == (H.HEC_OK, 0x1F, 2, H.CORRECT_UNLOCATED)
    assert np.array_equal(np.stack(units), before)
    coder.close()


def test_out_may_be_null(case):
    codec, k, m, coder = case
    truth = _copies(codec, k, m, 4099)
    units = [u.copy() for u in truth]
    units[k][77] ^= 0x33
    rc, r0, r1, unit = _correct_raw(coder, units, with_out=False)
    assert (rc, r0, r1) == (H.HEC_OK, 0xDEAD, 0xBEEF)
    assert unit == (k if m > 1 else H.CORRECT_UNLOCATED)
    if m > 1:
        assert np.array_equal(np.stack(units), np.stack(truth))


def test_bad_arguments():
    k, m = 6, 3
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    units = _copies("rs", k, m, 64)
    units[2][5] ^= 1
    before = np.stack(units)
    ptrs = [u.ctypes.data for u in units]
    res = (ctypes.c_uint64 * 2)(7, 7)
    unit = ctypes.c_int(77)
    lib = coder._lib
    call = lib.hec_scrub_correct
    assert call(coder.handle, H._pp(ptrs), 0, res, ctypes.byref(unit)) == H.HEC_ERR_INVALID_ARG
    assert call(coder.handle, H._pp(ptrs), 64, res, None) == H.HEC_ERR_INVALID_ARG
    assert call(coder.handle, None, 64, res, ctypes.byref(unit)) == H.HEC_ERR_INVALID_ARG
    assert call(None, H._pp(ptrs), 64, res, ctypes.byref(unit)) == H.HEC_ERR_INVALID_ARG
    for t in (0, k, k + m - 1):
        assert call(coder.handle, H._pp([0 if i == t else p for i, p in enumerate(ptrs)]), 64, res,
                    ctypes.byref(unit)) == H.HEC_ERR_INVALID_ARG
    assert (res[0], res[1], unit.value) == (7, 7, 77)  # untouched on error
    assert np.array_equal(np.stack(units), before)
    # the device call needs a device; its own argument checks come first for a NULL coder
    units_out = (ctypes.c_int32 * 1)(77)
    dev = lib.hec_scrub_correct_device
    assert dev(coder.handle, H._pp(ptrs), H._sp([64] * (k + m)), 64, 1, res, units_out, None) == H.HEC_ERR_DEVICE
    assert dev(None, H._pp(ptrs), H._sp([64] * (k + m)), 64, 1, res, units_out, None) == H.HEC_ERR_INVALID_ARG
    with pytest.raises(H.DeviceError):
        coder.scrub_correct_device(ptrs, [64] * (k + m), 64, 1, ctypes.addressof(res), ctypes.addressof(units_out))
    assert units_out[0] == 77 and np.array_equal(np.stack(units), before)
    coder.close()


def test_coder_method_round_trip():
    k, m = 10, 4
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    truth = [u[:777].tobytes() for u in _stripe("rs", k, m)]
    units = [bytearray(u) for u in truth]
    assert coder.scrub_correct(units) == (0, 0, H.CORRECT_CLEAN)
    units[12][300] ^= 0x55
    assert coder.scrub_correct(units) == (((1 << 14) - 1) & ~(1 << 12), 1, 12)
    assert [bytes(u) for u in units] == truth
    assert coder.scrub(units) == (0, 0)
    # writable numpy arrays are taken as they are; read-only buffers are refused
    arrs = [np.frombuffer(u, dtype=np.uint8).copy() for u in truth]
    arrs[3][:] = 0
    assert coder.scrub_correct(arrs)[2] == 3
    assert [a.tobytes() for a in arrs] == truth
    with pytest.raises(AssertionError):
        coder.scrub_correct(truth)
    with pytest.raises(AssertionError):
        coder.scrub_correct(units[:-1])
    coder.close()


# ---- C++ mirror, the sanitizer driver -------------------------------------------

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
CSRC = os.path.join(PKG_DIR, "csrc")


def _make(target, sources):
    """The Makefile's target, rebuilt only when missing or older than its sources."""
    binary = os.path.join(PKG_DIR, target)
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in sources):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, target])
    return binary


def test_cpp_mirror_scrub_correct():
    binary = _make("build/test_scrub_correct_mirror",
                   [os.path.join(ROOT, "tests", "cpp", "test_scrub_correct_mirror.cpp"),
                    os.path.join(CSRC, "hdfs_ec.hpp"), HEADER])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK 27" in r.stdout


def test_host_routine_sanitizer_driver():
    """host_gf.cpp and its driver in one program under AddressSanitizer + UBSan
    (linked statically; plain where the runtime is not installed): units in
    exact-size malloc blocks at every length above, every ISA this CPU has."""
    binary = _make("build/scrub_correct_host_check",
                   [os.path.join(ROOT, "tests", "cpp", "scrub_correct_host_check.cpp"),
                    os.path.join(CSRC, "host_gf.cpp"), os.path.join(CSRC, "host_gf.hpp"),
                    os.path.join(CSRC, "gf256.hpp")])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
