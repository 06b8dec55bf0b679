"""Degraded scrub on the CPU (hec_scrub_plan / hec_scrub_degraded): a stripe
with missing units -- are the units it still has consistent, and which one is
wrong?  Host-only coders; NULL slots are passed as NULL.  Expected results come
from degraded_scrub_ref.ref_scrub (rebuild-and-compare over the oracle's matrix
routines, not the engine's syndromes and minors); comparisons are exact."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import degraded_scrub_ref as R
import ec_oracle as O
import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT

BLOCK = 65536  # the host routine's block
LENS = (1, 37, BLOCK + 5)
SHAPES = [("rs", 6, 3), ("rs", 10, 4)]

_STRIPES = {}


def _stripe(codec, k, m):
    """A consistent stripe at the longest length (computed once)."""
    key = (codec, k, m)
    if key not in _STRIPES:
        rng = np.random.default_rng(9100 + 100 * k + m + len(codec))
        data = [rng.integers(0, 256, size=max(LENS), dtype=np.uint8) for _ in range(k)]
        _STRIPES[key] = data + O.matmul_shards(O.codec_matrix(codec, k, m)[k:], data)
    return _STRIPES[key]


def _copies(codec, k, m, length):
    return [np.ascontiguousarray(u[:length]).copy() for u in _stripe(codec, k, m)]


def _degraded_raw(coder, units, mask, length=None):
    """hec_scrub_degraded with the slots outside `mask` NULL: (status, ruled_out, bad_bytes)."""
    n = len(units[0]) if length is None else length
    ptrs = [u.ctypes.data if (mask >> i) & 1 else 0 for i, u in enumerate(units)]
    res = (ctypes.c_uint64 * 2)(0xDEAD, 0xBEEF)
    rc = coder._lib.hec_scrub_degraded(coder.handle, H._pp(ptrs), n, res)
    return rc, int(res[0]), int(res[1])


def _masks(k, m, rng):
    """Nothing lost, every single loss and a sample of double losses."""
    n = k + m
    full = (1 << n) - 1
    doubles = list(itertools.combinations(range(n), 2))
    picks = [doubles[i] for i in rng.choice(len(doubles), size=8, replace=False)]
    return [full] + [full & ~(1 << t) for t in range(n)] + [full & ~(1 << a) & ~(1 << b) for a, b in picks]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def case(request):
    codec, k, m = request.param
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    yield codec, k, m, coder
    coder.close()


@pytest.mark.parametrize("codec,k,m", [("rs", 3, 2), ("rs", 6, 3), ("rs", 10, 4), ("rs-legacy", 6, 3), ("xor", 3, 1)])
def test_plan_matches_oracle(codec, k, m):
    n = k + m
    full = (1 << n) - 1
    C = O.codec_matrix(codec, k, m)
    for lost_n in range(m + 1):
        for lost in itertools.combinations(range(n), lost_n):
            mask = full
            for t in lost:
                mask &= ~(1 << t)
            want = R.oracle_plan(codec, k, m, mask)
            got = H.scrub_plan(k, m, [(mask >> i) & 1 for i in range(n)], codec=codec)
            assert got == (want[0], want[1], [list(r) for r in want[2]]), (codec, lost)
            assert len(got[1]) == m - lost_n
            if lost_n == 0:
                assert got == (list(range(k)), list(range(k, n)), [list(r) for r in C[k:]])  # G = P
            # what lets the register kernel pivot its minors on row 0
            assert all(v != 0 for v in (got[2][0] if got[2] else []))


def test_plan_n_checks_and_errors():
    k, m = 6, 3
    e = ctypes.c_size_t(77)
    surv = (ctypes.c_size_t * k)(*([99] * k))

    def run(pres, codec=b"rs"):
        arr = (ctypes.c_uint8 * (k + m))(*pres)
        return H.lib.hec_scrub_plan(codec, k, m, arr, ctypes.byref(e), surv, None, None)

    assert run([1] * 6 + [0] * 3) == H.HEC_OK and e.value == 0  # exactly k present
    assert list(surv) == [99] * k  # nothing else is written
    assert run([1] * 4 + [0] * 5) == H.HEC_OK and e.value == 0  # fewer than k
    assert run([0, 1, 1, 1, 1, 1, 1, 1, 0]) == H.HEC_OK and e.value == 1
    assert list(surv) == [1, 2, 3, 4, 5, 6]
    assert run([1] * 9, b"nope") == H.HEC_ERR_UNSUPPORTED_CODEC
    assert H.lib.hec_scrub_plan(b"rs", k, m, None, ctypes.byref(e), None, None, None) == H.HEC_ERR_INVALID_ARG
    arr = (ctypes.c_uint8 * (k + m))(*([1] * 9))
    assert H.lib.hec_scrub_plan(b"rs", k, m, arr, None, None, None, None) == H.HEC_ERR_INVALID_ARG


def test_clean_stripe_any_loss(case):
    codec, k, m, coder = case
    rng = np.random.default_rng(1)
    for length in LENS:
        units = _copies(codec, k, m, length)
        for mask in _masks(k, m, rng):
            assert _degraded_raw(coder, units, mask) == (H.HEC_OK, 0, 0), (length, hex(mask))
            if length == 37:
                assert R.ref_scrub(codec, k, m, units, mask) == (0, 0)


@pytest.mark.parametrize("kind", ["survivor-byte", "extra-byte", "whole-unit", "two-units"])
def test_corruption_matches_reference(case, kind):
    codec, k, m, coder = case
    n = k + m
    rng = np.random.default_rng(len(kind) + k)
    for length in LENS:
        for mask in _masks(k, m, rng):
            units = _copies(codec, k, m, length)
            pres = R.present_units(n, mask)
            S, E = pres[:k], pres[k:]
            pos = int(rng.integers(0, length))
            if kind == "survivor-byte":
                hit = [S[int(rng.integers(0, k))]]
                units[hit[0]][pos] ^= int(rng.integers(1, 256))
            elif kind == "extra-byte":
                hit = [E[int(rng.integers(0, len(E)))]]
                units[hit[0]][pos] ^= int(rng.integers(1, 256))
            elif kind == "whole-unit":
                hit = [pres[int(rng.integers(0, len(pres)))]]
                units[hit[0]][:] = rng.integers(0, 256, size=length, dtype=np.uint8)
            else:
                hit = [int(t) for t in rng.choice(pres, size=2, replace=False)]
                units[hit[0]][pos] ^= int(rng.integers(1, 256))
                units[hit[1]][length - 1 - pos] ^= int(rng.integers(1, 256))
            want = R.ref_scrub(codec, k, m, units, mask)
            assert _degraded_raw(coder, units, mask) == (H.HEC_OK,) + want, (kind, length, hex(mask), hit)
            missing = ~mask & ((1 << n) - 1)
            if kind in ("survivor-byte", "extra-byte"):
                # the closed form: one bad position, the corrupt unit never ruled out
                assert want[1] == 1 and not (want[0] >> hit[0]) & 1 and want[0] & missing == missing
                verdict = H.scrub_verdict(want[0], want[1], n)
                if len(E) >= 2:
                    assert verdict == (H.HEC_SCRUB_LOCATED, hit[0])
                else:
                    assert verdict == (H.HEC_SCRUB_AMBIGUOUS, None)  # one check cannot locate
            elif kind == "two-units" and len(E) >= 3 and want[1] == 2:
                # (10,4) with one unit lost: two corrupt units cannot pass for one
                assert H.scrub_verdict(want[0], want[1], n) == (H.HEC_SCRUB_MULTIPLE, None)
            # two corrupt units with e == 2 may name a third: LOCATED assumes one (include/hdfs_ec_amd.h)


def test_two_corrupt_units_e3_is_multiple():
    codec, k, m = "rs", 10, 4
    n = k + m
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    try:
        for lost in (0, 7, 13):
            mask = ((1 << n) - 1) & ~(1 << lost)
            units = _copies(codec, k, m, 37)
            a, b = [t for t in range(n) if t != lost][2:9:6]
            units[a][5] ^= 0x11
            units[b][5] ^= 0x22  # the same position: a vector off every column
            rc, ruled, bad = _degraded_raw(coder, units, mask)
            assert (rc, bad) == (H.HEC_OK, 1)
            assert (ruled, bad) == R.ref_scrub(codec, k, m, units, mask)
            assert H.scrub_verdict(ruled, bad, n) == (H.HEC_SCRUB_MULTIPLE, None)
    finally:
        coder.close()


@pytest.mark.parametrize("codec,k,m", [("rs", 3, 2), ("rs", 6, 3), ("rs", 10, 4), ("xor", 5, 1), ("rs-legacy", 6, 3)])
def test_nothing_missing_equals_hec_scrub(codec, k, m):
    n = k + m
    full = (1 << n) - 1
    rng = np.random.default_rng(5 + k)
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    try:
        for length in LENS:
            units = _copies(codec, k, m, length)
            for step in range(4):
                res = (ctypes.c_uint64 * 2)(1, 2)
                assert coder._lib.hec_scrub(coder.handle, H._pp([u.ctypes.data for u in units]), length, res) == 0
                assert _degraded_raw(coder, units, full) == (H.HEC_OK, int(res[0]), int(res[1])), (length, step)
                assert coder.scrub_degraded(units) == (int(res[0]), int(res[1]))
                t = int(rng.integers(0, n))  # one more unit goes bad each step
                units[t][int(rng.integers(0, length))] ^= int(rng.integers(1, 256))
    finally:
        coder.close()


def test_unchecked_stripes_give_zero(case):
    codec, k, m, coder = case
    n = k + m
    units = _copies(codec, k, m, 37)
    for u in units:
        u[3] ^= 0xFF  # every unit is wrong: an unchecked stripe still reports nothing
    full = (1 << n) - 1
    exactly_k = full >> m  # the parity units lost
    assert _degraded_raw(coder, units, exactly_k) == (H.HEC_OK, 0, 0)
    assert _degraded_raw(coder, units, exactly_k & ~1) == (H.HEC_OK, 0, 0)  # fewer than k
    assert _degraded_raw(coder, units, 0) == (H.HEC_OK, 0, 0)
    assert R.ref_scrub(codec, k, m, units, exactly_k) == (0, 0)
    assert coder.scrub_degraded([None] * m + [u for u in units[m:]]) == (0, 0)


def test_invalid_arguments(case):
    codec, k, m, coder = case
    units = _copies(codec, k, m, 37)
    ptrs = H._pp([u.ctypes.data for u in units])
    res = (ctypes.c_uint64 * 2)(0xDEAD, 0xBEEF)
    f = coder._lib.hec_scrub_degraded
    assert f(None, ptrs, 37, res) == H.HEC_ERR_INVALID_ARG
    assert f(coder.handle, None, 37, res) == H.HEC_ERR_INVALID_ARG
    assert f(coder.handle, ptrs, 0, res) == H.HEC_ERR_INVALID_ARG
    assert f(coder.handle, ptrs, 37, None) == H.HEC_ERR_INVALID_ARG
    assert (res[0], res[1]) == (0xDEAD, 0xBEEF)
    # the device call on a host-only coder
    assert coder._lib.hec_scrub_device_mixed(coder.handle, ptrs, H._sp([37] * (k + m)),
                                             (ctypes.c_uint64 * 1)(1), 37, 1, res, None, 0,
                                             None) == H.HEC_ERR_DEVICE
    assert coder.scrub_mixed_workspace_size(100) > 0


def test_cpp_mirror_scrub_degraded():
    sources = [os.path.join(ROOT, "tests", "cpp", "test_scrub_degraded_mirror.cpp"),
               os.path.join(PKG_DIR, "csrc", "hdfs_ec.hpp"), os.path.join(ROOT, "include", "hdfs_ec_amd.h")]
    target = "build/test_scrub_degraded_mirror"
    binary = os.path.join(PKG_DIR, target)
    # the Makefile's target, rebuilt only when missing or older than its sources
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in sources):
        subprocess.check_call(["make", "-s", "-C", PKG_DIR, target])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK 72" in r.stdout
