"""Reconstruction of any lost unit of a stripe, parity included
(hec_reconstruct_plan / hec_reconstruct; Hadoop RSRawDecoder.decode), on the
CPU: the plan against the oracle's matrix algebra, the host routine against
the original stripe, the C++ mirror and the stand-alone C driver.  The ground
truth everywhere is the stripe that was encoded; comparisons are exact."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
from conftest import PKG_DIR, ROOT

CODECS = [("rs", 3, 2), ("rs", 6, 3), ("rs", 10, 4), ("xor", 5, 1), ("rs-legacy", 6, 3)]
LENS = (1, 15, 16, 17, 64, 4099)


def _patterns(n, lo, hi):
    """Every set of lo..hi lost unit indices out of n."""
    return [lost for e in range(lo, hi + 1) for lost in itertools.combinations(range(n), e)]


def _expected_plan(C, k, m, lost):
    """The issue's algebra with the oracle's helpers: survivors = first k
    present; data unit t -> row t of the inverse, parity unit k+j -> C[k+j] .
    inverse."""
    survivors = [i for i in range(k + m) if i not in lost][:k]
    inv = O.invert(O.select_rows(C, survivors))
    rows = [inv[t] if t < k else O.matmul([C[t]], inv)[0] for t in sorted(lost)]
    return survivors, sorted(lost), rows


@pytest.mark.parametrize("codec,k,m", CODECS)
def test_plan_every_pattern(codec, k, m):
    n = k + m
    C = O.codec_matrix(codec, k, m)
    for lost in _patterns(n, 0, m + 1):
        present = [i not in lost for i in range(n)]
        if len(lost) > m:
            with pytest.raises(H.ErasureCodingError):
                H.reconstruct_plan(k, m, present, codec=codec)
            continue
        got = H.reconstruct_plan(k, m, present, codec=codec)
        if not lost:
            assert got == ([], [], [])
            continue
        want = _expected_plan(C, k, m, lost)
        assert got == tuple(want), (codec, lost)
        # data rows are the decode plan's, byte for byte
        d_surv, d_miss, d_rows = H.decode_plan(k, m, present) if codec == "rs" else O.decode_plan(k, m, present, codec)
        if d_miss:
            assert d_surv == got[0] and d_miss == [t for t in got[1] if t < k]
            assert [list(r) for r in d_rows] == got[2][:len(d_miss)], (codec, lost)


def test_plan_nothing_wanted_with_too_few_present():
    # n_targets == 0 is "nothing to do" even when fewer than k units are present
    k, m = 6, 3
    present = [0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert H.reconstruct_plan(k, m, present, want=[]) == ([], [], [])
    with pytest.raises(H.ErasureCodingError):
        H.reconstruct_plan(k, m, present, want=[2])


def test_plan_want_subset():
    k, m = 6, 3
    C = O.gen_rs_matrix(k, m)
    present = [i not in (1, 7) for i in range(k + m)]
    surv, targets, rows = _expected_plan(C, k, m, (1, 7))
    assert H.reconstruct_plan(k, m, present, want=[7]) == (surv, [7], [rows[1]])
    assert H.reconstruct_plan(k, m, present, want=[1]) == (surv, [1], [rows[0]])
    assert H.reconstruct_plan(k, m, present, want=[1, 7]) == (surv, targets, rows)
    with pytest.raises(ValueError):  # HEC_ERR_INVALID_ARG: unit 0 is present
        H.reconstruct_plan(k, m, present, want=[0, 7])


def test_plan_rejects_bad_args():
    n = ctypes.c_size_t(0)
    pres = (ctypes.c_uint8 * 9)(*[1] * 9)
    assert H.lib.hec_reconstruct_plan(b"rs", 6, 3, None, None, ctypes.byref(n), None, None, None) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_reconstruct_plan(b"rs", 0, 3, pres, None, ctypes.byref(n), None, None, None) == H.HEC_ERR_INVALID_ARG
    assert H.lib.hec_reconstruct_plan(b"lrc", 6, 3, pres, None, ctypes.byref(n), None, None,
                                      None) == H.HEC_ERR_UNSUPPORTED_CODEC
    assert H.lib.hec_reconstruct_plan(b"xor", 6, 3, pres, None, ctypes.byref(n), None, None, None) == H.HEC_ERR_INVALID_ARG


# ---- host coder -----------------------------------------------------------

_STRIPES = {}


def _stripe(codec, k, m):
    """The original stripe at the longest length (computed once, read-only):
    random data and the oracle's parity; a shorter shard is a prefix."""
    key = (codec, k, m)
    if key not in _STRIPES:
        rng = np.random.default_rng(1000 * k + m)
        data = [rng.integers(0, 256, size=max(LENS), dtype=np.uint8) for _ in range(k)]
        units = data + O.matmul_shards(O.codec_matrix(codec, k, m)[k:], data)
        for u in units:
            u.setflags(write=False)
        _STRIPES[key] = units
    return _STRIPES[key]


def _reconstruct_raw(coder, units, lost, length, want=None, null_out=()):
    """hec_reconstruct on exact-length copies; every out buffer is handed in
    filled with 0xA5 (except null_out).  Returns (status, outs)."""
    n = len(units)
    ins = [None if i in lost else np.ascontiguousarray(units[i][:length]) for i in range(n)]
    outs = [np.full(length, 0xA5, dtype=np.uint8) for _ in range(n)]
    wb = None if want is None else (ctypes.c_uint8 * n)(*[1 if i in want else 0 for i in range(n)])
    rc = coder._lib.hec_reconstruct(coder.handle, H._pp([0 if a is None else a.ctypes.data for a in ins]), length, wb,
                                    H._pp([0 if i in null_out else outs[i].ctypes.data for i in range(n)]))
    return rc, outs


def _check_host(codec, k, m, patterns, lens=LENS):
    units = _stripe(codec, k, m)
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
    try:
        for lost in patterns:
            for length in lens:
                rc, outs = _reconstruct_raw(coder, units, lost, length)
                assert rc == H.HEC_OK, (lost, length, rc)
                for i in range(k + m):
                    if i in lost:
                        assert np.array_equal(outs[i], units[i][:length]), (codec, lost, length, i)
                    else:
                        assert (outs[i] == 0xA5).all(), (codec, lost, length, i)
    finally:
        coder.close()


def test_host_rs63_every_pattern():
    _check_host("rs", 6, 3, _patterns(9, 0, 3))


def test_host_rs104_sample():
    pats = _patterns(14, 1, 4)
    rng = np.random.default_rng(104)
    picks = [pats[i] for i in rng.choice(len(pats), size=60, replace=False)]
    _check_host("rs", 10, 4, picks + [(10, 11, 12, 13), (0, 1, 2, 3), (9, 13)])


def test_host_rs66_five_and_six_lost():
    rng = np.random.default_rng(66)
    for e in (5, 6):
        pats = _patterns(12, e, e)
        picks = [pats[i] for i in rng.choice(len(pats), size=25, replace=False)]
        _check_host("rs", 6, 6, picks + [tuple(range(6, 6 + e)), tuple(range(e))])


@pytest.mark.parametrize("codec,k,m", [("xor", 5, 1), ("rs-legacy", 6, 3)])
def test_host_other_codecs(codec, k, m):
    _check_host(codec, k, m, _patterns(k + m, 1, m), lens=(17, 4099))


def test_host_want_and_errors():
    k, m = 6, 3
    units = _stripe("rs", k, m)
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    for length in LENS:
        # two lost, one wanted: only that one is written
        rc, outs = _reconstruct_raw(coder, units, (2, 8), length, want=(8,), null_out=(2,))
        assert rc == H.HEC_OK
        assert np.array_equal(outs[8], units[8][:length])
        assert all((outs[i] == 0xA5).all() for i in range(k + m) if i != 8)
        # want on a present unit
        rc, outs = _reconstruct_raw(coder, units, (2, 8), length, want=(0, 8))
        assert rc == H.HEC_ERR_INVALID_ARG and all((o == 0xA5).all() for o in outs)
        # NULL out at a target
        rc, outs = _reconstruct_raw(coder, units, (2, 8), length, null_out=(8,))
        assert rc == H.HEC_ERR_INVALID_ARG and all((o == 0xA5).all() for o in outs)
        # fewer than k present: nothing written
        rc, outs = _reconstruct_raw(coder, units, (0, 3, 6, 7), length)
        assert rc == H.HEC_ERR_NOT_ENOUGH_SHARDS and all((o == 0xA5).all() for o in outs)
        # ... unless nothing is wanted
        rc, outs = _reconstruct_raw(coder, units, (0, 3, 6, 7), length, want=())
        assert rc == H.HEC_OK and all((o == 0xA5).all() for o in outs)
    # shard_len 0 is invalid, as for hec_encode
    rc, _ = _reconstruct_raw(coder, units, (2,), 0)
    assert rc == H.HEC_ERR_INVALID_ARG
    coder.close()


def test_host_coder_method_fills_slots_in_place():
    k, m = 10, 4
    units = [u[:777].tobytes() for u in _stripe("rs", k, m)]
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    shards = list(units)
    for i in (3, 9, 10, 13):
        shards[i] = None
    coder.reconstruct(shards)
    assert shards == units
    shards[4] = shards[12] = None
    coder.reconstruct(shards, want=[12])
    assert shards[12] == units[12] and shards[4] is None
    with pytest.raises(ValueError):
        coder.reconstruct(shards, want=[0])
    for i in (0, 1, 2, 3):
        shards[i] = None
    with pytest.raises(H.ErasureCodingError):
        coder.reconstruct(shards)
    coder.close()


def test_decode_calls_see_the_same_plans():
    """One cached plan now carries the rows of every lost unit; hec_decode on
    the same coder, before and after a reconstruct of the same mask, still
    rebuilds data units only and leaves parity slots alone."""
    k, m = 6, 3
    units = [u[:100].tobytes() for u in _stripe("rs", k, m)]
    coder = H.Coder(k, m, H.HEC_DEVICE_HOST)
    for _ in range(2):
        shards = list(units)
        shards[1] = shards[7] = None
        coder.decode(shards)
        assert shards[1] == units[1] and shards[7] is None
        shards[1] = None
        coder.reconstruct(shards)
        assert shards == units
    coder.close()


def test_mixed_workspace_size_is_bounded():
    """Only the fused kernel reads the workspace, and only when the plans fit
    its LDS: the size stops growing with the stripe count beyond the offsets."""
    c = H.Coder(10, 4, H.HEC_DEVICE_HOST)
    small, big = c.reconstruct_mixed_workspace_size(64), c.reconstruct_mixed_workspace_size(100_000)
    c.close()
    assert small >= 64 * 4 + 64 * (64 + 4 * 10 * 32) + 16 * 8 * 256  # 64 four-unit plans (84 KiB) fit whole
    assert big <= 100_000 * 4 + (156 << 10) + 16 * 8 * 256 + 2 * 256  # offsets + resident LDS + counters + padding


# ---- C++ mirror and the stand-alone C driver --------------------------------

def _build(binary, compiler_args, sources):
    # a direct compile line (the drivers link the engine dynamically); rebuilt
    # only when missing or older than its sources
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in sources):
        os.makedirs(os.path.dirname(binary), exist_ok=True)
        subprocess.check_call(compiler_args + ["-o", binary, sources[0], "-L" + os.path.join(PKG_DIR, "lib"),
                                               "-lhdfs_ec_amd", "-Wl,-rpath,$ORIGIN/../lib"])
    return binary


HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")


@pytest.fixture(scope="module")
def mirror_binary():
    return _build(os.path.join(PKG_DIR, "build", "test_reconstruct_mirror"),
                  ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread"],
                  [os.path.join(ROOT, "tests", "cpp", "test_reconstruct_mirror.cpp"),
                   os.path.join(PKG_DIR, "csrc", "hdfs_ec.hpp"), HEADER])


@pytest.fixture(scope="module")
def check_binary():
    return _build(os.path.join(PKG_DIR, "build", "reconstruct_check"), ["gcc", "-O2", "-std=c11", "-Wall", "-Wextra"],
                  [os.path.join(ROOT, "tests", "cpp", "reconstruct_check.c"), HEADER])


def test_cpp_mirror_reconstruct(mirror_binary):
    r = subprocess.run([mirror_binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK 129" in r.stdout


def test_standalone_driver(check_binary):
    r = subprocess.run([check_binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
