"""Stripe scrub on the CPU (hec_scrub / hec_scrub_verdict; `hdfs debug
verifyEC`): are the k+m units of a stripe consistent, and if not, which one is
wrong?  Expected results come from _ref_scrub below, a numpy restatement of
the definition (syndromes s_j = sum_i P[j][i] u_i ^ u_{k+j}; ruled_out bit t
when some position's syndrome vector has a non-zero 2x2 minor against column t
of H = [P | I]) over the oracle's matrix and product table; comparisons are
exact.  Then the C++ mirror, the stand-alone C driver and the host routine's
sanitizer driver."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT

CODECS = [("rs", 3, 2), ("rs", 6, 3), ("rs", 10, 4), ("xor", 5, 1), ("rs-legacy", 6, 3)]
BLOCK = 65536  # the host routine's block: 65536 + 17 crosses it
LENS = (1, 15, 16, 17, 64, 4099, BLOCK + 17)


def _ref_scrub(C, k, m, units):
    """(ruled_out, bad_bytes) of one stripe by the definition."""
    P = np.array(C[k:], dtype=np.uint8)
    Hm = np.concatenate([P, np.eye(m, dtype=np.uint8)], axis=1)  # m x (k+m)
    s = np.stack([np.array(units[k + j], dtype=np.uint8) for j in range(m)])
    for j in range(m):
        for i in range(k):
            s[j] ^= O.MUL_TABLE[P[j, i]][units[i]]
    bad = np.nonzero(s.any(axis=0))[0]
    sb = s[:, bad]
    ruled = 0
    for t in range(k + m):
        for i in range(m):
            for j in range(i + 1, m):
                if (O.MUL_TABLE[Hm[j, t]][sb[i]] ^ O.MUL_TABLE[Hm[i, t]][sb[j]]).any():
                    ruled |= 1 << t
    return ruled, len(bad)


_STRIPES = {}


def _stripe(codec, k, m):
    """A consistent stripe at the longest length (computed once); a shorter
    stripe is a prefix of every unit."""
    key = (codec, k, m)
    if key not in _STRIPES:
        rng = np.random.default_rng(7000 + 100 * k + m + len(codec))
        data = [rng.integers(0, 256, size=max(LENS), dtype=np.uint8) for _ in range(k)]
        _STRIPES[key] = data + O.matmul_shards(O.codec_matrix(codec, k, m)[k:], data)
    return _STRIPES[key]


def _scrub_raw(coder, units, length=None):
    """hec_scrub on the given arrays; returns (status, ruled_out, bad_bytes)."""
    n = len(units[0]) if length is None else length
    res = (ctypes.c_uint64 * 2)(0xDEAD, 0xBEEF)
    rc = coder._lib.hec_scrub(coder.handle, H._pp([u.ctypes.data for u in units]), n, res)
    return rc, int(res[0]), int(res[1])


@pytest.fixture(scope="module", params=CODECS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def case(request):
    codec, k, m = request.param
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    yield codec, k, m, coder, O.codec_matrix(codec, k, m)
    coder.close()


def _copies(codec, k, m, length):
    return [np.ascontiguousarray(u[:length]).copy() for u in _stripe(codec, k, m)]


def test_parity_block_has_no_zero(case):
    # what lets the device kernel's fast path use the minors against row 0 alone
    _, k, _, _, C = case
    assert all(v != 0 for row in C[k:] for v in row)


def test_clean_stripe(case):
    codec, k, m, coder, C = case
    for length in LENS:
        units = _copies(codec, k, m, length)
        assert _scrub_raw(coder, units) == (H.HEC_OK, 0, 0), length
        assert _ref_scrub(C, k, m, units) == (0, 0)


def test_one_flipped_bit_names_its_unit(case):
    codec, k, m, coder, C = case
    n = k + m
    full = (1 << n) - 1
    for length in LENS:
        units = _copies(codec, k, m, length)
        for pos in sorted({0, length - 1, BLOCK - 1, BLOCK}):
            if pos >= length:
                continue
            for t in range(n):
                units[t][pos] ^= 1 << (t % 8)
                want = (full & ~(1 << t), 1) if m > 1 else (0, 1)
                assert _scrub_raw(coder, units) == (H.HEC_OK,) + want, (codec, length, pos, t)
                if length in (17, BLOCK + 17) and t in (0, n - 1):
                    assert _ref_scrub(C, k, m, units) == want  # the restatement agrees with the closed form
                if m > 1:
                    assert H.scrub_verdict(*want, n) == (H.HEC_SCRUB_LOCATED, t)
                else:
                    assert H.scrub_verdict(*want, n) == (H.HEC_SCRUB_AMBIGUOUS, None)
                units[t][pos] ^= 1 << (t % 8)


def test_random_unit(case):
    codec, k, m, coder, C = case
    rng = np.random.default_rng(11)
    for length in LENS:
        units = _copies(codec, k, m, length)
        for t in (0, k - 1, k, k + m - 1):
            keep = units[t].copy()
            units[t][:] = rng.integers(0, 256, size=length, dtype=np.uint8)
            want = _ref_scrub(C, k, m, units)
            assert _scrub_raw(coder, units) == (H.HEC_OK,) + want, (codec, length, t)
            if m > 1 and length >= 16:  # (a random byte equals the original one time in 256)
                assert 0 < want[1] <= length and H.scrub_verdict(*want, k + m) == (H.HEC_SCRUB_LOCATED, t)
            units[t][:] = keep


def test_two_units_two_positions(case):
    codec, k, m, coder, C = case
    n = k + m
    for length in LENS[1:]:
        units = _copies(codec, k, m, length)
        units[1][0] ^= 0x40
        units[n - 1][length - 1] ^= 0x02
        want = _ref_scrub(C, k, m, units)
        assert want == (((1 << n) - 1) if m > 1 else 0, 2)
        assert _scrub_raw(coder, units) == (H.HEC_OK,) + want, (codec, length)
        assert H.scrub_verdict(*want, n)[0] == (H.HEC_SCRUB_MULTIPLE if m > 1 else H.HEC_SCRUB_AMBIGUOUS)


def test_two_units_one_position(case):
    codec, k, m, coder, C = case
    n = k + m
    rng = np.random.default_rng(5)
    for length in LENS:
        units = _copies(codec, k, m, length)
        pos = length // 2
        for a, b in ((0, 1), (k - 1, k), (k, n - 1), (0, n - 1)):
            if a == b:
                continue
            ea, eb = (int(v) for v in rng.integers(1, 256, size=2))
            units[a][pos] ^= ea
            units[b][pos] ^= eb
            want = _ref_scrub(C, k, m, units)
            if m >= 3:  # two corrupt units can never pass for one
                assert want == ((1 << n) - 1, 1), (codec, a, b)
            assert _scrub_raw(coder, units) == (H.HEC_OK,) + want, (codec, length, a, b)
            units[a][pos] ^= ea
            units[b][pos] ^= eb


def test_verdict():
    full = (1 << 9) - 1
    assert H.scrub_verdict(0, 0, 9) == (H.HEC_SCRUB_CLEAN, None)
    assert H.scrub_verdict(full, 0, 9) == (H.HEC_SCRUB_CLEAN, None)  # bad_bytes decides
    for t in range(9):
        assert H.scrub_verdict(full & ~(1 << t), 3, 9) == (H.HEC_SCRUB_LOCATED, t)
    assert H.scrub_verdict(full, 2, 9) == (H.HEC_SCRUB_MULTIPLE, None)
    assert H.scrub_verdict(full & ~0b11, 2, 9) == (H.HEC_SCRUB_AMBIGUOUS, None)
    assert H.scrub_verdict(0, 1, 6) == (H.HEC_SCRUB_AMBIGUOUS, None)  # m = 1
    assert H.scrub_verdict(full, 1, 10) == (H.HEC_SCRUB_LOCATED, 9)  # bits >= units are outside the stripe
    assert H.scrub_verdict((1 << 63) - 1, 1, 64) == (H.HEC_SCRUB_LOCATED, 63)
    # `unit` is written only for LOCATED
    unit = ctypes.c_int(-7)
    for ruled, bad in ((0, 0), (full, 2), (full & ~0b11, 2)):
        assert H.lib.hec_scrub_verdict(ruled, bad, 9, ctypes.byref(unit)) != H.HEC_SCRUB_LOCATED
        assert unit.value == -7
    assert H.lib.hec_scrub_verdict(full & ~4, 1, 9, ctypes.byref(unit)) == H.HEC_SCRUB_LOCATED and unit.value == 2
    assert H.lib.hec_scrub_verdict(full & ~4, 1, 9, None) == H.HEC_SCRUB_LOCATED
    for units in (0, 65, 1 << 20):
        assert H.lib.hec_scrub_verdict(0, 1, units, ctypes.byref(unit)) == H.HEC_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            H.scrub_verdict(0, 1, units)


def test_bad_arguments():
    k, m = 6, 3
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    units = _copies("rs", k, m, 64)
    ptrs = [u.ctypes.data for u in units]
    res = (ctypes.c_uint64 * 2)(7, 7)
    lib = coder._lib
    assert lib.hec_scrub(coder.handle, H._pp(ptrs), 0, res) == H.HEC_ERR_INVALID_ARG
    assert lib.hec_scrub(coder.handle, H._pp(ptrs), 64, None) == H.HEC_ERR_INVALID_ARG
    assert lib.hec_scrub(coder.handle, None, 64, res) == H.HEC_ERR_INVALID_ARG
    assert lib.hec_scrub(None, H._pp(ptrs), 64, res) == H.HEC_ERR_INVALID_ARG
    for t in (0, k, k + m - 1):
        assert lib.hec_scrub(coder.handle, H._pp([0 if i == t else p for i, p in enumerate(ptrs)]), 64,
                             res) == H.HEC_ERR_INVALID_ARG
    assert (res[0], res[1]) == (7, 7)  # untouched on error
    # the device call needs a device
    assert lib.hec_scrub_device(coder.handle, H._pp(ptrs), H._sp([64] * (k + m)), 64, 1, res, None) == H.HEC_ERR_DEVICE
    assert lib.hec_scrub_device(None, H._pp(ptrs), H._sp([64] * (k + m)), 64, 1, res, None) == H.HEC_ERR_INVALID_ARG
    coder.close()


def test_host_limit_does_not_route_scrub_away():
    # hec_scrub is the host routine whatever the limit (0 = "always the device"
    # for hec_encode): a host-only coder still answers
    coder = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    coder.host_limit = 0
    units = _copies("rs", 6, 3, 4099)
    units[4][100] ^= 9
    assert _scrub_raw(coder, units) == (H.HEC_OK, 0x1FF & ~(1 << 4), 1)
    coder.close()


def test_coder_method_round_trip():
    k, m = 10, 4
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    units = [u[:777].tobytes() for u in _stripe("rs", k, m)]
    assert coder.scrub(units) == (0, 0)
    assert H.scrub_verdict(*coder.scrub(units), k + m) == (H.HEC_SCRUB_CLEAN, None)
    bad = list(units)
    bad[12] = bad[12][:300] + bytes([bad[12][300] ^ 0x55]) + bad[12][301:]
    got = coder.scrub(bad)
    assert got == (((1 << 14) - 1) & ~(1 << 12), 1)
    assert H.scrub_verdict(*got, k + m) == (H.HEC_SCRUB_LOCATED, 12)
    # numpy arrays are taken as they are
    assert coder.scrub([np.frombuffer(b, dtype=np.uint8) for b in bad]) == got
    with pytest.raises(AssertionError):
        coder.scrub(units[:-1])
    coder.close()


# ---- C++ mirror, the stand-alone C driver, the sanitizer driver ---------------

HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
CSRC = os.path.join(PKG_DIR, "csrc")


def _make(target, sources):
    """The Makefile's target, rebuilt only when missing or older than its sources."""
    binary = os.path.join(PKG_DIR, target)
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in sources):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, target])
    return binary


def test_cpp_mirror_scrub():
    binary = _make("build/test_scrub_mirror", [os.path.join(ROOT, "tests", "cpp", "test_scrub_mirror.cpp"),
                                               os.path.join(CSRC, "hdfs_ec.hpp"), HEADER])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK 18" in r.stdout


def test_standalone_driver():
    binary = _make("build/scrub_check", [os.path.join(ROOT, "tests", "cpp", "scrub_check.c"), HEADER])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def test_host_routine_sanitizer_driver():
    """host_gf.cpp and its driver in one program under AddressSanitizer + UBSan
    (linked statically; plain where the runtime is not installed): exact-length
    heap units at every length above, every ISA this CPU has."""
    binary = _make("build/scrub_host_check", [os.path.join(ROOT, "tests", "cpp", "scrub_host_check.cpp"),
                                              os.path.join(CSRC, "host_gf.cpp"), os.path.join(CSRC, "host_gf.hpp"),
                                              os.path.join(CSRC, "gf256.hpp")])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
