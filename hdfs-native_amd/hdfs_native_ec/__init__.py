"""ctypes binding of the MI355X EC engine's C ABI (include/hdfs_ec_amd.h).

Mirrors the reference's Rust surface so parity tests read like the
reference's own tests:

  hdfs_native::ec::gf256::Coder::new(data_units, parity_units)   gf256.rs:32-38
  Coder::gen_rs_matrix(k, m)                                     gf256.rs:40-57
  Coder::encode(&[Bytes]) -> Vec<Bytes>                          gf256.rs:61-80
  Coder::decode(&mut [Option<Bytes>]) -> Result<()>              gf256.rs:84-137

plus the batched device-resident entry points used by bench.py.  There is no
CPU fallback anywhere: if lib/libhdfs_ec_amd.so is missing or fails to load,
import raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HEC_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libhdfs_ec_amd.so")
# HEC_LIB_PATH: another in-tree build of the engine, for same-box A/B measurements

HEC_OK = 0
HEC_ERR_INVALID_ARG = -1
HEC_ERR_NOT_ENOUGH_SHARDS = -2
HEC_ERR_UNSUPPORTED_CODEC = -3
HEC_ERR_DEVICE = -4
HEC_ERR_NO_MEMORY = -5
HEC_ERR_SINGULAR = -6
HEC_ERR_CHECKSUM = -7
HEC_DEVICE_HOST = -2  # host-only coder: the engine's host routine, no GPU needed

# hec_scrub_verdict outcomes
HEC_SCRUB_CLEAN = 0
HEC_SCRUB_LOCATED = 1
HEC_SCRUB_AMBIGUOUS = 2
HEC_SCRUB_MULTIPLE = 3

# hec_scrub_correct[_device]: the unit values that are not a unit index
CORRECT_CLEAN = -1      # HEC_CORRECT_CLEAN: bad_bytes == 0, stripe untouched
CORRECT_UNLOCATED = -2  # HEC_CORRECT_UNLOCATED: AMBIGUOUS or MULTIPLE, stripe untouched

# ChecksumTypeProto values (rust/src/proto/hadoop.hdfs.rs:1363)
CHECKSUM_NULL = 0
CHECKSUM_CRC32 = 1   # crc CRC_32_CKSUM (connection.rs:37)
CHECKSUM_CRC32C = 2  # crc CRC_32_ISCSI (connection.rs:38)

# Every symbol include/hdfs_ec_amd.h declares (checked by tests/test_capi.py).
EXPORTS = [
    "hec_strerror", "hec_abi_version", "hec_last_error", "hec_gen_rs_matrix", "hec_matrix_invert",
    "hec_gen_codec_matrix",
    "hec_decode_plan", "hec_coder_create", "hec_coder_destroy", "hec_coder_data_units",
    "hec_coder_parity_units", "hec_coder_device", "hec_encode", "hec_decode",
    "hec_encode_device", "hec_decode_device", "hec_gf_matmul_device",
    "hec_encode_host_batch", "hec_decode_mixed_workspace_size",
    "hec_decode_device_mixed", "hec_coder_create_codec", "hec_decode_host_batch",
    "hec_crc32c_device", "hec_encode_crc_device", "hec_checksum_device", "hec_checksum_verify_device",
    "hec_decode_verify_device", "hec_group_create", "hec_group_destroy", "hec_group_size", "hec_group_coder",
    "hec_group_range", "hec_group_encode_host_batch", "hec_group_decode_host_batch", "hec_group_encode_device",
    "hec_group_decode_device",
    "hec_device_alloc", "hec_device_free", "hec_device_copy", "hec_device_synchronize", "hec_device_numa_node",
    "hec_host_alloc", "hec_host_free",
    "hec_coder_acquire", "hec_coder_release", "hec_coder_pool_trim", "hec_coder_set_host_limit",
    "hec_coder_host_limit", "hec_gf_matmul_host", "hec_host_isa", "hec_encode_rows_host",
    "hec_coder_prepare_decode", "hec_jit_warm", "hec_jit_stats", "hec_queue_stats",
    "hec_encode_rows_workspace_size", "hec_encode_rows_device", "hec_decode_rows_host",
    "hec_reconstruct_plan", "hec_reconstruct", "hec_reconstruct_device",
    "hec_reconstruct_mixed_workspace_size", "hec_reconstruct_device_mixed",
    "hec_reconstruct_crc_device", "hec_reconstruct_crc_mixed_workspace_size", "hec_reconstruct_crc_device_mixed",
    "hec_reconstruct_sums_device", "hec_reconstruct_sums_device_mixed",
    "hec_reconstruct_crc_rows_device", "hec_reconstruct_crc_rows_mixed_workspace_size",
    "hec_reconstruct_crc_rows_device_mixed",
    "hec_scrub_verdict", "hec_scrub", "hec_scrub_device", "hec_scrub_correct", "hec_scrub_correct_device",
    "hec_scrub_plan", "hec_scrub_degraded", "hec_scrub_mixed_workspace_size", "hec_scrub_device_mixed",
    "hec_scrub_crc_device", "hec_scrub_crc_mixed_workspace_size", "hec_scrub_crc_device_mixed",
    "hec_scrub_crc_rows_device", "hec_scrub_crc_rows_mixed_workspace_size", "hec_scrub_crc_rows_device_mixed",
    "hec_encode_crc_rows_device", "hec_encode_crc_rows_mixed_workspace_size", "hec_encode_crc_rows_device_mixed",
    "hec_read_crc_rows_device", "hec_read_crc_rows_mixed_workspace_size", "hec_read_crc_rows_device_mixed",
    "hec_crc_concat", "hec_composite_crc", "hec_composite_crc_workspace_size", "hec_composite_crc_device",
]


class HdfsError(Exception):
    """Base of the errors the reference reports (rust/src/error.rs)."""


class ErasureCodingError(HdfsError):
    """HdfsError::ErasureCodingError (error.rs:34-35)."""


class UnsupportedErasureCodingPolicy(HdfsError):
    """HdfsError::UnsupportedErasureCodingPolicy (error.rs:32-33)."""


class ChecksumError(HdfsError):
    """HdfsError::ChecksumError (error.rs; raised by ReadPacket::get_data,
    connection.rs:497-499)."""


class DeviceError(HdfsError):
    pass


def _share_torch_hip_runtime() -> None:
    """If PyTorch is installed, import it BEFORE loading the engine.

    torch's wheel bundles its own libamdhip64 and links it by the unversioned
    name; our .so links libamdhip64.so.7.  Loaded lib-first, the process ends
    up with two HIP runtimes and whichever initialises first owns the GPU
    (the other reports "no ROCm-capable device").  Loaded torch-first, our
    DT_NEEDED libamdhip64.so.7 matches the SONAME of torch's copy and one
    runtime serves both.  Set HEC_NO_TORCH_PRELOAD=1 to skip."""
    import importlib.util
    if os.environ.get("HEC_NO_TORCH_PRELOAD") == "1":
        return
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


EXP_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libhdfs_ec_amd_exp.so")


def _load(path: str = LIB_PATH) -> ctypes.CDLL:
    _share_torch_hip_runtime()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not built: run `make -C hdfs-native_amd` (or __graft_entry__.build()). "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    P, S, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    PP = ctypes.POINTER(ctypes.c_void_p)
    SP = ctypes.POINTER(ctypes.c_size_t)
    sig = {
        "hec_strerror": ([I], ctypes.c_char_p),
        "hec_abi_version": ([], I),
        "hec_last_error": ([], ctypes.c_char_p),
        "hec_gen_rs_matrix": ([S, S, P], I),
        "hec_gen_codec_matrix": ([ctypes.c_char_p, S, S, P], I),
        "hec_matrix_invert": ([P, S], I),
        "hec_decode_plan": ([S, S, P, SP, SP, SP, P], I),
        "hec_coder_create": ([S, S, I, ctypes.POINTER(P)], I),
        "hec_coder_create_codec": ([ctypes.c_char_p, S, S, I, ctypes.POINTER(P)], I),
        "hec_coder_destroy": ([P], None),
        "hec_coder_data_units": ([P], S),
        "hec_coder_parity_units": ([P], S),
        "hec_coder_device": ([P], I),
        "hec_encode": ([P, PP, S, PP], I),
        "hec_decode": ([P, PP, S, PP], I),
        "hec_encode_device": ([P, PP, SP, PP, SP, S, S, P], I),
        "hec_decode_device": ([P, PP, SP, PP, SP, S, S, P], I),
        "hec_gf_matmul_device": ([P, P, S, S, PP, SP, PP, SP, S, S, P], I),
        "hec_encode_host_batch": ([P, P, P, S, S, S], I),
        "hec_decode_host_batch": ([P, PP, S, S, P, S], I),
        "hec_crc32c_device": ([P, PP, SP, S, S, S, S, P, P], I),
        "hec_encode_crc_device": ([P, PP, SP, PP, SP, S, S, S, P, P], I),
        "hec_checksum_device": ([P, I, PP, SP, S, S, S, S, P, P], I),
        "hec_checksum_verify_device": ([P, I, PP, SP, S, S, S, S, P, P, P], I),
        "hec_decode_verify_device": ([P, I, PP, SP, PP, SP, S, S, S, P, P, P], I),
        "hec_decode_mixed_workspace_size": ([P, S], S),
        "hec_decode_device_mixed": ([P, PP, SP, PP, SP, ctypes.POINTER(ctypes.c_uint64), S, S, P, S, P], I),
        "hec_group_create": ([ctypes.c_char_p, S, S, ctypes.POINTER(I), S, ctypes.POINTER(P)], I),
        "hec_group_destroy": ([P], None),
        "hec_group_size": ([P], S),
        "hec_group_coder": ([P, S], P),
        "hec_group_range": ([P, S, S, SP, SP], I),
        "hec_group_encode_host_batch": ([P, P, P, S, S, S], I),
        "hec_group_decode_host_batch": ([P, PP, S, S, P, S], I),
        "hec_group_encode_device": ([P, PP, SP, PP, SP, S, SP, PP], I),
        "hec_group_decode_device": ([P, PP, SP, PP, SP, S, SP, PP], I),
        "hec_device_alloc": ([I, S, ctypes.c_uint, ctypes.POINTER(P)], I),
        "hec_device_free": ([I, P], I),
        "hec_device_numa_node": ([I], I),
        "hec_device_copy": ([I, P, P, S], I),
        "hec_device_synchronize": ([I, P], I),
        "hec_host_alloc": ([I, S, I, ctypes.POINTER(P)], I),
        "hec_host_free": ([P], I),
        "hec_coder_acquire": ([ctypes.c_char_p, S, S, I, ctypes.POINTER(P)], I),
        "hec_coder_release": ([P], None),
        "hec_coder_pool_trim": ([], S),
        "hec_coder_set_host_limit": ([P, S], I),
        "hec_coder_host_limit": ([P], S),
        "hec_coder_prepare_decode": ([P, P, I, P], I),
        "hec_jit_warm": ([S, S, P, I], I),
        "hec_jit_stats": ([P, P, P, P], None),
        "hec_queue_stats": ([I, P, P, P], None),
        "hec_gf_matmul_host": ([P, S, S, PP, PP, S], I),
        "hec_host_isa": ([], ctypes.c_char_p),
        "hec_encode_rows_host": ([P, P, S, P, S, S], I),
        "hec_encode_rows_workspace_size": ([P, S], S),
        "hec_encode_rows_device": ([P, P, S, P, S, P, S, P], I),
        "hec_decode_rows_host": ([P, PP, SP, S, P, S, S], I),
        "hec_reconstruct_plan": ([ctypes.c_char_p, S, S, P, P, SP, SP, SP, P], I),
        "hec_reconstruct": ([P, PP, S, P, PP], I),
        "hec_reconstruct_device": ([P, PP, SP, PP, SP, P, S, S, P], I),
        "hec_reconstruct_mixed_workspace_size": ([P, S], S),
        "hec_reconstruct_device_mixed": ([P, PP, SP, PP, SP, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64), S, S, P, S, P], I),
        "hec_reconstruct_crc_device": ([P, I, PP, SP, PP, SP, P, S, S, S, P, P, P, P], I),
        "hec_reconstruct_crc_mixed_workspace_size": ([P, S], S),
        "hec_reconstruct_crc_device_mixed": ([P, I, PP, SP, PP, SP, ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, P, P, S, P], I),
        "hec_reconstruct_sums_device": ([P, I, PP, SP, P, S, S, S, ctypes.c_uint64, P, P, P, P], I),
        "hec_reconstruct_sums_device_mixed": ([P, I, PP, SP, ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, P, P, S, P], I),
        "hec_reconstruct_crc_rows_device": ([P, I, PP, SP, PP, SP, P, S, S, S, ctypes.c_uint64, P, P, P, P], I),
        "hec_reconstruct_crc_rows_mixed_workspace_size": ([P, S], S),
        "hec_reconstruct_crc_rows_device_mixed": ([P, I, PP, SP, PP, SP, ctypes.POINTER(ctypes.c_uint64),
                                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                   S, S, S, P, P, P, P, S, P], I),
        "hec_scrub_verdict": ([ctypes.c_uint64, ctypes.c_uint64, S, ctypes.POINTER(I)], I),
        "hec_scrub": ([P, PP, S, P], I),
        "hec_scrub_device": ([P, PP, SP, S, S, P, P], I),
        "hec_scrub_correct": ([P, PP, S, P, ctypes.POINTER(I)], I),
        "hec_scrub_correct_device": ([P, PP, SP, S, S, P, P, P], I),
        "hec_scrub_plan": ([ctypes.c_char_p, S, S, P, SP, SP, SP, P], I),
        "hec_scrub_degraded": ([P, PP, S, P], I),
        "hec_scrub_mixed_workspace_size": ([P, S], S),
        "hec_scrub_device_mixed": ([P, PP, SP, ctypes.POINTER(ctypes.c_uint64), S, S, P, P, S, P], I),
        "hec_scrub_crc_device": ([P, I, PP, SP, S, S, S, P, P, P, P], I),
        "hec_scrub_crc_mixed_workspace_size": ([P, S], S),
        "hec_scrub_crc_device_mixed": ([P, I, PP, SP, ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, P, P, S, P], I),
        "hec_scrub_crc_rows_device": ([P, I, PP, SP, S, S, S, ctypes.c_uint64, P, P, P, P], I),
        "hec_scrub_crc_rows_mixed_workspace_size": ([P, S], S),
        "hec_scrub_crc_rows_device_mixed": ([P, I, PP, SP, ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, P, P, S, P], I),
        "hec_encode_crc_rows_device": ([P, I, PP, SP, PP, SP, S, S, S, ctypes.c_uint64, P, P], I),
        "hec_encode_crc_rows_mixed_workspace_size": ([P, S], S),
        "hec_encode_crc_rows_device_mixed": ([P, I, PP, SP, PP, SP, ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, S,
                                              P], I),
        "hec_read_crc_rows_device": ([P, I, PP, SP, P, S, S, S, S, ctypes.c_uint64, P, P, P], I),
        "hec_read_crc_rows_mixed_workspace_size": ([P, S], S),
        "hec_read_crc_rows_device_mixed": ([P, I, PP, SP, P, S, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint64), S, S, S, P, P, P, S, P], I),
        "hec_crc_concat": ([I, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)], I),
        "hec_composite_crc": ([I, P, S, S, S, S, S, ctypes.c_uint64, P, P, P], I),
        "hec_composite_crc_workspace_size": ([S, S], S),
        "hec_composite_crc_device": ([P, I, P, S, S, S, S, S, ctypes.c_uint64, P, P, P, P, S, P], I),
    }
    if hasattr(lib, "hec_tune_set"):  # the measurement build only (include/hdfs_ec_amd_exp.h)
        sig["hec_tune_set"] = ([I, I], I)
    for name, (args, res) in sig.items():
        if os.environ.get("HEC_LIB_PATH") and not hasattr(lib, name):
            continue  # an older build loaded for a same-box A/B: entry points it predates stay unbound
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


lib = _load()
_exp_lib = None


def experimental_available() -> bool:
    return os.path.exists(EXP_LIB_PATH)


def experimental_lib() -> ctypes.CDLL:
    """The HEC_EXPERIMENTAL measurement build (lib/libhdfs_ec_amd_exp.so,
    `make -C hdfs-native_amd exp`: the default kernels plus every shape a knob
    can select and the measured-and-rejected variants).  Pass it as
    Coder(..., lib=experimental_lib()); its knobs (include/hdfs_ec_amd_exp.h)
    are its own.  The product library has no knobs."""
    global _exp_lib
    if _exp_lib is None:
        if not experimental_available():
            raise ImportError(f"{EXP_LIB_PATH} not built: run `make -C hdfs-native_amd exp` (measurement build)")
        _exp_lib = _load(EXP_LIB_PATH)
    return _exp_lib


def strerror(rc: int) -> str:
    return lib.hec_strerror(rc).decode()


def _check(rc: int) -> None:
    if rc == HEC_OK:
        return
    msg = strerror(rc)
    if rc == HEC_ERR_NOT_ENOUGH_SHARDS:
        raise ErasureCodingError("Not enough valid shards")
    if rc == HEC_ERR_UNSUPPORTED_CODEC:
        raise UnsupportedErasureCodingPolicy(msg)
    if rc == HEC_ERR_CHECKSUM:
        raise ChecksumError(msg)
    if rc in (HEC_ERR_INVALID_ARG, HEC_ERR_SINGULAR):
        raise ValueError(msg)
    if rc == HEC_ERR_NO_MEMORY:
        raise MemoryError(msg)
    raise DeviceError(f"{msg} (status {rc}): {lib.hec_last_error().decode()}")


def _pp(addrs: Sequence[int]):
    return (ctypes.c_void_p * len(addrs))(*addrs)


def _sp(vals: Sequence[int]):
    return (ctypes.c_size_t * len(vals))(*vals)


def gen_rs_matrix(data_units: int, parity_units: int) -> List[List[int]]:
    buf = (ctypes.c_uint8 * ((data_units + parity_units) * data_units))()
    _check(lib.hec_gen_rs_matrix(data_units, parity_units, buf))
    k = data_units
    return [list(buf[r * k:(r + 1) * k]) for r in range(data_units + parity_units)]


def gen_codec_matrix(codec: str, data_units: int, parity_units: int) -> List[List[int]]:
    """The (k+m) x k matrix a coder of `codec` ("rs", "xor", "rs-legacy") uses."""
    buf = (ctypes.c_uint8 * ((data_units + parity_units) * data_units))()
    _check(lib.hec_gen_codec_matrix(codec.encode(), data_units, parity_units, buf))
    k = data_units
    return [list(buf[r * k:(r + 1) * k]) for r in range(data_units + parity_units)]


def matrix_invert(mat: List[List[int]]) -> List[List[int]]:
    n = len(mat)
    buf = (ctypes.c_uint8 * (n * n))(*[v for row in mat for v in row])
    _check(lib.hec_matrix_invert(buf, n))
    return [list(buf[r * n:(r + 1) * n]) for r in range(n)]


def host_isa() -> str:
    """The host routine's ISA (hec_host_isa): avx512bw+gfni, avx2 or scalar."""
    return lib.hec_host_isa().decode()


def gf_matmul_host(matrix: List[List[int]], shards: Sequence) -> List[bytes]:
    """hec_gf_matmul_host: the hot loop Mul<&[&[u8]]> (matrix.rs:204-231) on
    the host -- out[j] = sum_i matrix[j][i] * shards[i] over GF(2^8)."""
    import numpy as np
    rows, cols = len(matrix), len(matrix[0])
    ins = [np.ascontiguousarray(np.frombuffer(bytes(x) if not isinstance(x, np.ndarray) else x, dtype=np.uint8))
           for x in shards]
    n = len(ins[0])
    outs = [np.empty(n, dtype=np.uint8) for _ in range(rows)]
    mat = (ctypes.c_uint8 * (rows * cols))(*[v for r in matrix for v in r])
    _check(lib.hec_gf_matmul_host(mat, rows, cols, _pp([a.ctypes.data for a in ins]),
                                  _pp([a.ctypes.data for a in outs]), n))
    return [o.tobytes() for o in outs]


def pool_trim() -> int:
    """hec_coder_pool_trim: destroys the idle pooled coders."""
    return lib.hec_coder_pool_trim()


def decode_plan(data_units: int, parity_units: int, present: Sequence[bool]):
    k, m = data_units, parity_units
    pres = (ctypes.c_uint8 * (k + m))(*[1 if p else 0 for p in present])
    e = ctypes.c_size_t(0)
    surv = (ctypes.c_size_t * k)()
    miss = (ctypes.c_size_t * k)()
    mat = (ctypes.c_uint8 * (k * k))()
    _check(lib.hec_decode_plan(k, m, pres, ctypes.byref(e), surv, miss, mat))
    e = e.value
    return list(surv) if e else [], list(miss[:e]), [list(mat[r * k:(r + 1) * k]) for r in range(e)]


def _want_bytes(n: int, want):
    """want: None (every missing unit) or the unit indices to rebuild."""
    if want is None:
        return None
    w = set(want)
    return (ctypes.c_uint8 * n)(*[1 if i in w else 0 for i in range(n)])


def reconstruct_plan(data_units: int, parity_units: int, present: Sequence[bool], want=None, codec: str = "rs"):
    """hec_reconstruct_plan: (survivors, targets, matrix) for rebuilding the
    missing units of `present` (data or parity); `want` = unit indices to
    rebuild (None = every missing unit)."""
    k, m = data_units, parity_units
    pres = (ctypes.c_uint8 * (k + m))(*[1 if p else 0 for p in present])
    t = ctypes.c_size_t(0)
    surv = (ctypes.c_size_t * k)()
    targ = (ctypes.c_size_t * (k + m))()
    mat = (ctypes.c_uint8 * ((k + m) * k))()
    _check(lib.hec_reconstruct_plan(codec.encode(), k, m, pres, _want_bytes(k + m, want), ctypes.byref(t), surv,
                                    targ, mat))
    t = t.value
    return list(surv) if t else [], list(targ[:t]), [list(mat[r * k:(r + 1) * k]) for r in range(t)]


def scrub_plan(data_units: int, parity_units: int, present: Sequence[bool], codec: str = "rs"):
    """hec_scrub_plan: (survivors, extras, matrix) of the degraded scrub of a
    stripe with the units of `present`: the first k present units, the other e
    present units and G = C[extras] . inverse(C[survivors]) as e rows.  e == 0
    (k units present or fewer: nothing to check against) gives ([], [], [])."""
    k, m = data_units, parity_units
    pres = (ctypes.c_uint8 * (k + m))(*[1 if p else 0 for p in present])
    e = ctypes.c_size_t(0)
    surv = (ctypes.c_size_t * k)()
    extras = (ctypes.c_size_t * m)()
    mat = (ctypes.c_uint8 * (m * k))()
    _check(lib.hec_scrub_plan(codec.encode(), k, m, pres, ctypes.byref(e), surv, extras, mat))
    e = e.value
    return list(surv) if e else [], list(extras[:e]), [list(mat[r * k:(r + 1) * k]) for r in range(e)]


def scrub_verdict(ruled_out: int, bad_bytes: int, units: int):
    """hec_scrub_verdict: (verdict, unit) for one stripe's scrub result over
    `units` = k+m units; unit is the located unit for HEC_SCRUB_LOCATED, else
    None.  LOCATED is exact for up to m-1 corrupt units when m >= 3 and assumes
    at most one when m == 2 (include/hdfs_ec_amd.h)."""
    unit = ctypes.c_int(-1)
    rc = lib.hec_scrub_verdict(ruled_out, bad_bytes, units, ctypes.byref(unit))
    if rc < 0:
        _check(rc)
    return rc, (unit.value if rc == HEC_SCRUB_LOCATED else None)


ALLOC_DEFAULT = 0
ALLOC_CONTIGUOUS = 1


def crc_concat(checksum_type: int, crc_a: int, crc_b: int, len_b: int) -> int:
    """crc(A || B) from crc(A), crc(B) and |B| (hec_crc_concat)."""
    out = ctypes.c_uint32()
    _check(lib.hec_crc_concat(checksum_type, crc_a, crc_b, len_b, ctypes.byref(out)))
    return out.value


def composite_crc_workspace_size(n_units: int, stripes: int) -> int:
    return lib.hec_composite_crc_workspace_size(n_units, stripes)


def composite_crc(checksum_type: int, sums, n_units: int, data_units: int, cell_len: int, stripes: int,
                  bytes_per_checksum: int = 512, data_len: int = 0, want=("cell", "unit", "group")):
    """hec_composite_crc on the host: `sums` is the [stripes][n_units][nck]
    big-endian chunk-sum array (bytes-like).  Returns (cell_crcs, unit_crcs,
    group_crc): lists of ints ([stripes][n_units], [n_units]) and an int, None
    for an output not in `want`."""
    buf = (ctypes.c_uint8 * max(1, len(sums))).from_buffer_copy(bytes(sums) or b"\0")
    cell = (ctypes.c_uint8 * max(1, 4 * stripes * n_units))() if "cell" in want else None
    unit = (ctypes.c_uint8 * (4 * n_units))() if "unit" in want else None
    group = (ctypes.c_uint8 * 4)() if "group" in want else None
    _check(lib.hec_composite_crc(checksum_type, buf, n_units, data_units, cell_len, stripes, bytes_per_checksum,
                                 data_len, cell, unit, group))

    def words(b, count):
        return [int.from_bytes(bytes(b[4 * i:4 * i + 4]), "big") for i in range(count)]

    cells = None
    if cell is not None:
        flat = words(cell, stripes * n_units)
        cells = [flat[s * n_units:(s + 1) * n_units] for s in range(stripes)]
    return (cells, words(unit, n_units) if unit is not None else None,
            words(group, 1)[0] if group is not None else None)


class DeviceBuffer:
    """HBM from hec_device_alloc (optionally physically contiguous), exposed
    to torch through __cuda_array_interface__: `torch.as_tensor(buf,
    device=...)` views it without a copy.  Freed by close()."""

    def __init__(self, nbytes: int, device: int = 0, flags: int = ALLOC_DEFAULT):
        p = ctypes.c_void_p()
        _check(lib.hec_device_alloc(device, nbytes, flags, ctypes.byref(p)))
        self.ptr, self.nbytes, self.device = p.value, nbytes, device

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}

    def close(self) -> None:
        if self.ptr:
            _check(lib.hec_device_free(self.device, ctypes.c_void_p(self.ptr)))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory on a NUMA node (hec_host_alloc; numa_node -1
    = the node of `device`).  .array() views it as a numpy uint8 array."""

    def __init__(self, nbytes: int, device: int = 0, numa_node: int = -1):
        p = ctypes.c_void_p()
        _check(lib.hec_host_alloc(device, nbytes, numa_node, ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def array(self):
        import numpy as np
        return np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr))

    def close(self) -> None:
        if self.ptr:
            _check(lib.hec_host_free(ctypes.c_void_p(self.ptr)))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_numa_node(device: int = 0) -> int:
    return lib.hec_device_numa_node(device)


def tune_set(key: int, value: int, lib_=None) -> None:
    """hec_tune_set on the measurement build (default: experimental_lib())."""
    _check((lib_ or experimental_lib()).hec_tune_set(key, value))


def _addr(buf) -> int:
    """Address of a writable/readable contiguous host buffer (numpy array,
    bytearray, ctypes array, or bytes via a copy-free view when possible)."""
    import numpy as np
    if isinstance(buf, np.ndarray):
        assert buf.flags["C_CONTIGUOUS"]
        return buf.ctypes.data
    arr = np.frombuffer(buf, dtype=np.uint8)
    return arr.ctypes.data


class Coder:
    """Drop-in for hdfs_native::ec::gf256::Coder on one MI355X.  pooled=True
    takes the coder from the process-wide pool (hec_coder_acquire; device -1
    = any) and close() returns it (hec_coder_release)."""

    def __init__(self, data_units: int, parity_units: int, device: int = 0, codec: str = "rs", lib=None,
                 pooled: bool = False):
        self._lib = lib or globals()["lib"]
        h = ctypes.c_void_p()
        if pooled:
            _check(self._lib.hec_coder_acquire(codec.encode(), data_units, parity_units, device, ctypes.byref(h)))
            device = self._lib.hec_coder_device(h)
        else:
            _check(self._lib.hec_coder_create_codec(codec.encode(), data_units, parity_units, device,
                                                    ctypes.byref(h)))
        self.pooled = pooled
        self.codec = codec
        self._h = h
        self.data_units = data_units
        self.parity_units = parity_units
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            (self._lib.hec_coder_release if self.pooled else self._lib.hec_coder_destroy)(self._h)
            self._h = None

    @property
    def host_limit(self) -> int:
        """Rows of at most this many bytes per shard are coded on the host
        (hec_coder_host_limit); 0 = always the device."""
        return self._lib.hec_coder_host_limit(self._h)

    @host_limit.setter
    def host_limit(self, max_shard_len: int) -> None:
        _check(self._lib.hec_coder_set_host_limit(self._h, max_shard_len))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    gen_rs_matrix = staticmethod(gen_rs_matrix)

    # -- host-buffer API: Coder::encode / Coder::decode --------------------
    def encode(self, data: Sequence[bytes]) -> List[bytes]:
        """gf256.rs:61-80: returns m parity shards as bytes."""
        import numpy as np
        assert len(data) == self.data_units, "data.len() == data_units (gf256.rs:62)"
        n = len(data[0])
        assert all(len(d) == n for d in data), "equal shard lengths (gf256.rs:65)"
        ins = [np.ascontiguousarray(np.frombuffer(bytes(d) if not isinstance(d, np.ndarray) else d,
                                                  dtype=np.uint8)) for d in data]
        outs = [np.empty(n, dtype=np.uint8) for _ in range(self.parity_units)]
        _check(self._lib.hec_encode(self._h, _pp([a.ctypes.data for a in ins]), n,
                              _pp([a.ctypes.data for a in outs])))
        return [o.tobytes() for o in outs]

    def decode(self, data: List[Optional[bytes]]) -> None:
        """gf256.rs:84-137: fills missing data slots of `data` in place."""
        import numpy as np
        k, m = self.data_units, self.parity_units
        assert len(data) == k + m
        present = [d for d in data if d is not None]
        if not present:
            _check(HEC_ERR_NOT_ENOUGH_SHARDS if any(d is None for d in data[:k]) else HEC_OK)
            return
        n = len(present[0])
        ins = [None if d is None else np.ascontiguousarray(np.frombuffer(bytes(d), dtype=np.uint8))
               for d in data]
        outs = [np.empty(n, dtype=np.uint8) if (i < k and data[i] is None) else None for i in range(k + m)]
        _check(self._lib.hec_decode(self._h, _pp([0 if a is None else a.ctypes.data for a in ins]), n,
                              _pp([0 if a is None else a.ctypes.data for a in outs])))
        for i in range(k):
            if data[i] is None:
                data[i] = outs[i].tobytes()

    def reconstruct(self, data: List[Optional[bytes]], want=None) -> None:
        """hec_reconstruct: fills the missing slots of `data`, data or parity,
        in place (Hadoop RSRawDecoder.decode); `want` = the unit indices to
        rebuild (None = every missing one; the others stay None)."""
        import numpy as np
        n_units = self.data_units + self.parity_units
        assert len(data) == n_units
        present = [d for d in data if d is not None]
        targets = [i for i in range(n_units) if data[i] is None and (want is None or i in set(want))]
        if want is not None and any(data[i] is not None for i in want):
            _check(HEC_ERR_INVALID_ARG)
        if not present:
            _check(HEC_ERR_NOT_ENOUGH_SHARDS if targets else HEC_OK)
            return
        n = len(present[0])
        ins = [None if d is None else np.ascontiguousarray(np.frombuffer(bytes(d), dtype=np.uint8)) for d in data]
        outs = [np.empty(n, dtype=np.uint8) if i in targets else None for i in range(n_units)]
        _check(self._lib.hec_reconstruct(self._h, _pp([0 if a is None else a.ctypes.data for a in ins]), n,
                                         _want_bytes(n_units, want),
                                         _pp([0 if a is None else a.ctypes.data for a in outs])))
        for i in targets:
            data[i] = outs[i].tobytes()

    def scrub(self, shards: Sequence[bytes]):
        """hec_scrub: (ruled_out, bad_bytes) of one stripe whose k+m units are
        all present (host routine; see scrub_verdict)."""
        import numpy as np
        n_units = self.data_units + self.parity_units
        assert len(shards) == n_units
        n = len(shards[0])
        assert all(len(d) == n for d in shards), "equal shard lengths"
        ins = [np.ascontiguousarray(np.frombuffer(bytes(d) if not isinstance(d, np.ndarray) else d, dtype=np.uint8))
               for d in shards]
        res = (ctypes.c_uint64 * 2)()
        _check(self._lib.hec_scrub(self._h, _pp([a.ctypes.data for a in ins]), n, res))
        return int(res[0]), int(res[1])

    def scrub_device(self, shard_ptrs, shard_strides, cell_len, stripes, results_ptr, stream: int = 0) -> None:
        """hec_scrub_device: shard_ptrs[k+m] (none missing); results_ptr = device
        memory for `stripes` pairs of uint64 (ruled_out, bad_bytes), zeroed by the call."""
        _check(self._lib.hec_scrub_device(self._h, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides), cell_len,
                                          stripes, ctypes.c_void_p(results_ptr), ctypes.c_void_p(stream)))

    def scrub_correct(self, shards):
        """hec_scrub_correct: scrub one stripe of k+m writable buffers
        (bytearray, writable numpy uint8 arrays, ...) and, where one unit is
        LOCATED, fix it in place.  -> (ruled_out, bad_bytes, unit): the pair the
        scrub found and the corrected unit, CORRECT_CLEAN or CORRECT_UNLOCATED
        (nothing written).  Host routine."""
        import numpy as np
        n_units = self.data_units + self.parity_units
        assert len(shards) == n_units
        views = [np.frombuffer(d, dtype=np.uint8) for d in shards]
        n = len(views[0])
        assert all(len(v) == n for v in views), "equal shard lengths"
        assert all(v.flags.writeable for v in views), "writable buffers"
        res = (ctypes.c_uint64 * 2)()
        unit = ctypes.c_int(0)
        _check(self._lib.hec_scrub_correct(self._h, _pp([v.ctypes.data for v in views]), n, res, ctypes.byref(unit)))
        return int(res[0]), int(res[1]), unit.value

    def scrub_correct_device(self, shard_ptrs, shard_strides, cell_len, stripes, results_ptr, units_ptr,
                             stream: int = 0) -> None:
        """hec_scrub_correct_device: shard_ptrs[k+m] (none missing, writable);
        results_ptr = what scrub_device / scrub_crc_device wrote for these
        cells earlier on the stream; units_ptr = device memory for `stripes`
        int32 (the corrected unit, CORRECT_CLEAN or CORRECT_UNLOCATED),
        written for every stripe."""
        _check(self._lib.hec_scrub_correct_device(self._h, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides),
                                                  cell_len, stripes, ctypes.c_void_p(results_ptr),
                                                  ctypes.c_void_p(units_ptr), ctypes.c_void_p(stream)))

    def scrub_degraded(self, shards: Sequence[Optional[bytes]]):
        """hec_scrub_degraded: (ruled_out, bad_bytes) of one stripe, None =
        missing unit (host routine).  The missing units' bits are set in
        ruled_out once a position is bad; (0, 0) when k units or fewer are
        present (nothing to check against)."""
        import numpy as np
        n_units = self.data_units + self.parity_units
        assert len(shards) == n_units
        ins = [None if d is None else
               np.ascontiguousarray(np.frombuffer(bytes(d) if not isinstance(d, np.ndarray) else d, dtype=np.uint8))
               for d in shards]
        lens = {len(a) for a in ins if a is not None}
        assert len(lens) <= 1, "equal shard lengths"
        res = (ctypes.c_uint64 * 2)()
        _check(self._lib.hec_scrub_degraded(self._h, _pp([0 if a is None else a.ctypes.data for a in ins]),
                                            lens.pop() if lens else 0, res))
        return int(res[0]), int(res[1])

    def scrub_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_scrub_mixed_workspace_size(self._h, stripes)

    def scrub_device_mixed(self, shard_ptrs, shard_strides, present_masks, cell_len, stripes, results_ptr,
                           workspace_ptr, workspace_bytes, stream: int = 0) -> None:
        """hec_scrub_device_mixed: shard_ptrs[k+m] (none None), one presence
        mask per stripe; results_ptr as scrub_device, workspace_ptr = device
        memory of scrub_mixed_workspace_size(stripes) bytes."""
        masks = None if present_masks is None else (ctypes.c_uint64 * max(stripes, 1))(*present_masks)
        _check(self._lib.hec_scrub_device_mixed(self._h, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides), masks,
                                                cell_len, stripes, ctypes.c_void_p(results_ptr),
                                                ctypes.c_void_p(workspace_ptr), workspace_bytes,
                                                ctypes.c_void_p(stream)))

    def scrub_crc_device(self, shard_ptrs, shard_strides, cell_len, stripes, expected_ptr, bad_ptr, results_ptr,
                         bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                         stream: int = 0) -> None:
        """hec_scrub_crc_device: scrub_device with every unit's chunk sums
        verified in the same pass against expected_ptr ([stripe][k+m][nck]
        big-endian u32); a mismatch sets bad_ptr[stripe * (k+m) + unit] (flags
        zeroed by the caller).  results_ptr as scrub_device."""
        _check(self._lib.hec_scrub_crc_device(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                              _sp(shard_strides), cell_len, stripes, bytes_per_checksum,
                                              ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
                                              ctypes.c_void_p(results_ptr), ctypes.c_void_p(stream)))

    def scrub_crc_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_scrub_crc_mixed_workspace_size(self._h, stripes)

    def scrub_crc_device_mixed(self, shard_ptrs, shard_strides, present_masks, cell_len, stripes, expected_ptr,
                               bad_ptr, results_ptr, workspace_ptr, workspace_bytes, bytes_per_checksum: int = 512,
                               checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_scrub_crc_device_mixed: scrub_device_mixed with the checksum
        buffers of scrub_crc_device (only the present units are verified); the
        workspace is scrub_crc_mixed_workspace_size(stripes) bytes."""
        masks = None if present_masks is None else (ctypes.c_uint64 * max(stripes, 1))(*present_masks)
        _check(self._lib.hec_scrub_crc_device_mixed(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                    _sp(shard_strides), masks, cell_len, stripes, bytes_per_checksum,
                                                    ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
                                                    ctypes.c_void_p(results_ptr), ctypes.c_void_p(workspace_ptr),
                                                    workspace_bytes, ctypes.c_void_p(stream)))

    def scrub_crc_rows_device(self, shard_ptrs, shard_strides, cell_len, stripes, expected_ptr, bad_ptr, results_ptr,
                              data_len: int = 0, bytes_per_checksum: int = 512,
                              checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_scrub_crc_rows_device: scrub_crc_device for a group whose last
        stripe is short.  data_len as for composite_crc (0 = every stripe
        full): the last stripe is checked over its positions below n0 and
        every unit is verified over its own bytes."""
        _check(self._lib.hec_scrub_crc_rows_device(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                   _sp(shard_strides), cell_len, stripes, bytes_per_checksum,
                                                   data_len, ctypes.c_void_p(expected_ptr),
                                                   ctypes.c_void_p(bad_ptr), ctypes.c_void_p(results_ptr),
                                                   ctypes.c_void_p(stream)))

    def scrub_crc_rows_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_scrub_crc_rows_mixed_workspace_size(self._h, stripes)

    def scrub_crc_rows_device_mixed(self, shard_ptrs, shard_strides, present_masks, stripe_bytes, cell_len, stripes,
                                    expected_ptr, bad_ptr, results_ptr, workspace_ptr, workspace_bytes,
                                    bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                                    stream: int = 0) -> None:
        """hec_scrub_crc_rows_device_mixed: scrub_crc_device_mixed with the
        logical bytes of every stripe (stripe_bytes[s]; None = all full; 0 or
        k * cell_len = that stripe is full).  The workspace is
        scrub_crc_rows_mixed_workspace_size(stripes) bytes, 16-byte aligned."""
        masks = None if present_masks is None else (ctypes.c_uint64 * max(stripes, 1))(*present_masks)
        lens = None if stripe_bytes is None else (ctypes.c_uint64 * max(stripes, 1))(*stripe_bytes)
        _check(self._lib.hec_scrub_crc_rows_device_mixed(
            self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides), masks, lens, cell_len,
            stripes, bytes_per_checksum, ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
            ctypes.c_void_p(results_ptr), ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream)))

    def prepare_decode(self, missing: Sequence[int], checksum_type: int = 2) -> bool:
        """hec_coder_prepare_decode: compile the plan-specialised fused decode
        + verify kernel for shards `missing` unavailable, now; True when it
        is ready (see include/hdfs_ec_amd.h)."""
        n = self.data_units + self.parity_units
        present = (ctypes.c_uint8 * n)(*[0 if i in set(missing) else 1 for i in range(n)])
        flag = ctypes.c_int(0)
        _check(self._lib.hec_coder_prepare_decode(self._h, present, checksum_type, ctypes.byref(flag)))
        return bool(flag.value)

    # -- device-resident batched API ----------------------------------------
    def encode_device(self, data_ptrs, data_strides, parity_ptrs, parity_strides, cell_len, stripes,
                      stream: int = 0) -> None:
        _check(self._lib.hec_encode_device(self._h, _pp(data_ptrs), _sp(data_strides), _pp(parity_ptrs),
                                     _sp(parity_strides), cell_len, stripes, ctypes.c_void_p(stream)))

    def decode_device(self, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len, stripes,
                      stream: int = 0) -> None:
        _check(self._lib.hec_decode_device(self._h, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides),
                                     _pp([p or 0 for p in out_ptrs]), _sp(out_strides), cell_len, stripes,
                                     ctypes.c_void_p(stream)))

    def crc32c_device(self, ptrs, strides, cell_len, stripes, bytes_per_checksum, out_ptr, stream: int = 0):
        _check(self._lib.hec_crc32c_device(self._h, _pp(ptrs), _sp(strides), len(ptrs), cell_len, stripes,
                                     bytes_per_checksum, ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream)))

    def checksum_device(self, checksum_type: int, ptrs, strides, cell_len, stripes, bytes_per_checksum, out_ptr,
                        stream: int = 0):
        _check(self._lib.hec_checksum_device(self._h, checksum_type, _pp(ptrs), _sp(strides), len(ptrs), cell_len, stripes,
                                       bytes_per_checksum, ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream)))

    def checksum_verify_device(self, checksum_type: int, ptrs, strides, cell_len, stripes, bytes_per_checksum,
                               expected_ptr, bad_ptr, stream: int = 0):
        _check(self._lib.hec_checksum_verify_device(self._h, checksum_type, _pp(ptrs), _sp(strides), len(ptrs), cell_len,
                                              stripes, bytes_per_checksum, ctypes.c_void_p(expected_ptr),
                                              ctypes.c_void_p(bad_ptr), ctypes.c_void_p(stream)))

    def composite_crc_device(self, checksum_type: int, sums_ptr: int, n_units: int, data_units: int, cell_len: int,
                             stripes: int, bytes_per_checksum: int, data_len: int = 0, cell_crcs_ptr: int = 0,
                             unit_crcs_ptr: int = 0, group_crc_ptr: int = 0, workspace: int = 0,
                             workspace_bytes: int = 0, stream: int = 0) -> None:
        """hec_composite_crc_device: cell / unit / group CRCs (big-endian u32,
        each optional: 0 = not computed) from the chunk sums at sums_ptr,
        asynchronously on `stream`.  The workspace
        (composite_crc_workspace_size(n_units, stripes) bytes) is needed for
        the unit and group outputs."""
        _check(self._lib.hec_composite_crc_device(self._h, checksum_type, sums_ptr, n_units, data_units, cell_len,
                                                  stripes, bytes_per_checksum, data_len, cell_crcs_ptr or None,
                                                  unit_crcs_ptr or None, group_crc_ptr or None, workspace or None,
                                                  workspace_bytes, stream or None))

    def decode_verify_device(self, checksum_type: int, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len,
                             stripes, bytes_per_checksum, sums_ptr, bad_ptr, stream: int = 0) -> None:
        """Verified striped read (hec_decode_verify_device): raises
        ErasureCodingError when a stripe has fewer than k cells that verify
        (the bad flags are written either way)."""
        _check(self._lib.hec_decode_verify_device(self._h, checksum_type, _pp(shard_ptrs), _sp(shard_strides),
                                            _pp(out_ptrs), _sp(out_strides), cell_len, stripes, bytes_per_checksum,
                                            ctypes.c_void_p(sums_ptr), ctypes.c_void_p(bad_ptr),
                                            ctypes.c_void_p(stream)))

    def encode_crc_device(self, data_ptrs, data_strides, parity_ptrs, parity_strides, cell_len, stripes,
                          bytes_per_checksum, sums_ptr, stream: int = 0):
        _check(self._lib.hec_encode_crc_device(self._h, _pp(data_ptrs), _sp(data_strides), _pp(parity_ptrs),
                                         _sp(parity_strides), cell_len, stripes, bytes_per_checksum,
                                         ctypes.c_void_p(sums_ptr), ctypes.c_void_p(stream)))

    def encode_crc_rows_device(self, data_ptrs, data_strides, parity_ptrs, parity_strides, cell_len, stripes,
                               sums_ptr, data_len: int = 0, bytes_per_checksum: int = 512,
                               checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_encode_crc_rows_device: encode_crc_device with a checksum type
        for a group whose last stripe is short.  data_len as for composite_crc
        (0 = every stripe full): the last stripe's parity units get their n0 =
        min(cell, r) bytes, nothing at or past n0 is written, and every unit
        gets the sums of its own bytes."""
        _check(self._lib.hec_encode_crc_rows_device(
            self._h, checksum_type, None if data_ptrs is None else _pp([p or 0 for p in data_ptrs]),
            _sp(data_strides), None if parity_ptrs is None else _pp([p or 0 for p in parity_ptrs]),
            _sp(parity_strides), cell_len, stripes, bytes_per_checksum, data_len, ctypes.c_void_p(sums_ptr),
            ctypes.c_void_p(stream)))

    def encode_crc_rows_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_encode_crc_rows_mixed_workspace_size(self._h, stripes)

    def encode_crc_rows_device_mixed(self, data_ptrs, data_strides, parity_ptrs, parity_strides, stripe_bytes,
                                     cell_len, stripes, sums_ptr, workspace_ptr, workspace_bytes,
                                     bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                                     stream: int = 0) -> None:
        """hec_encode_crc_rows_device_mixed: the logical bytes of every stripe
        (stripe_bytes[s]; None = all full; 0 or k * cell_len = that stripe is
        full).  The workspace (encode_crc_rows_mixed_workspace_size(stripes)
        bytes, 8-byte aligned) is needed only when a stripe is short."""
        lens = None if stripe_bytes is None else (ctypes.c_uint64 * max(stripes, 1))(*stripe_bytes)
        _check(self._lib.hec_encode_crc_rows_device_mixed(
            self._h, checksum_type, None if data_ptrs is None else _pp([p or 0 for p in data_ptrs]),
            _sp(data_strides), None if parity_ptrs is None else _pp([p or 0 for p in parity_ptrs]),
            _sp(parity_strides), lens, cell_len, stripes, bytes_per_checksum, ctypes.c_void_p(sums_ptr),
            ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream)))

    def read_crc_rows_device(self, shard_ptrs, shard_strides, file_ptr, cell_len, stripes, file_stride: int = 0,
                             data_len: int = 0, expected_ptr=None, bad_ptr=None, bytes_per_checksum: int = 512,
                             checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_read_crc_rows_device: the verified striped read into a
        file-order buffer.  shard_ptrs[k+m] (None / 0 = lost for the batch);
        data unit u of stripe s goes to file_ptr + s * file_stride + u *
        cell_len (file_stride 0 = k * cell_len) for its own length, copied or
        rebuilt; data_len as for encode_crc_rows_device.  With expected_ptr the
        survivors are verified and bad_ptr's flags set."""
        _check(self._lib.hec_read_crc_rows_device(
            self._h, checksum_type, None if shard_ptrs is None else _pp([p or 0 for p in shard_ptrs]),
            None if shard_strides is None else _sp(shard_strides), ctypes.c_void_p(file_ptr), file_stride, cell_len,
            stripes, bytes_per_checksum, data_len, ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
            ctypes.c_void_p(stream)))

    def read_crc_rows_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_read_crc_rows_mixed_workspace_size(self._h, stripes)

    def read_crc_rows_device_mixed(self, shard_ptrs, shard_strides, file_ptr, present_masks, stripe_bytes, cell_len,
                                   stripes, workspace_ptr, workspace_bytes, file_stride: int = 0, expected_ptr=None,
                                   bad_ptr=None, bytes_per_checksum: int = 512,
                                   checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_read_crc_rows_device_mixed: read_crc_rows_device with one
        presence mask per stripe and the logical bytes of every stripe
        (stripe_bytes[s]; None = all full; 0 or k * cell_len = that stripe is
        full).  The workspace (read_crc_rows_mixed_workspace_size(stripes)
        bytes, 8-byte aligned) is always needed."""
        masks = None if present_masks is None else (ctypes.c_uint64 * max(stripes, 1))(*present_masks)
        lens = None if stripe_bytes is None else (ctypes.c_uint64 * max(stripes, 1))(*stripe_bytes)
        _check(self._lib.hec_read_crc_rows_device_mixed(
            self._h, checksum_type, None if shard_ptrs is None else _pp([p or 0 for p in shard_ptrs]),
            None if shard_strides is None else _sp(shard_strides), ctypes.c_void_p(file_ptr), file_stride, masks, lens,
            cell_len, stripes, bytes_per_checksum, ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
            ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream)))

    def decode_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_decode_mixed_workspace_size(self._h, stripes)

    def decode_device_mixed(self, shard_ptrs, shard_strides, out_ptrs, out_strides, present_masks, cell_len,
                            stripes, workspace_ptr, workspace_bytes, stream: int = 0) -> None:
        masks = (ctypes.c_uint64 * stripes)(*present_masks)
        _check(self._lib.hec_decode_device_mixed(self._h, _pp(shard_ptrs), _sp(shard_strides), _pp(out_ptrs),
                                           _sp(out_strides), masks, cell_len, stripes,
                                           ctypes.c_void_p(workspace_ptr), workspace_bytes,
                                           ctypes.c_void_p(stream)))

    def reconstruct_device(self, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len, stripes, want=None,
                           stream: int = 0) -> None:
        """hec_reconstruct_device: shard_ptrs[k+m] (None = missing), out_ptrs
        [k+m] (used at the targets; may be the lost unit's own slot)."""
        _check(self._lib.hec_reconstruct_device(self._h, _pp([p or 0 for p in shard_ptrs]), _sp(shard_strides),
                                                _pp([p or 0 for p in out_ptrs]), _sp(out_strides),
                                                _want_bytes(len(shard_ptrs), want), cell_len, stripes,
                                                ctypes.c_void_p(stream)))

    def reconstruct_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_reconstruct_mixed_workspace_size(self._h, stripes)

    def reconstruct_device_mixed(self, shard_ptrs, shard_strides, out_ptrs, out_strides, present_masks, want_masks,
                                 cell_len, stripes, workspace_ptr, workspace_bytes, stream: int = 0) -> None:
        """hec_reconstruct_device_mixed: per-stripe presence masks and (or
        None: everything missing) per-stripe masks of the units to rebuild."""
        masks = (ctypes.c_uint64 * stripes)(*present_masks)
        wants = None if want_masks is None else (ctypes.c_uint64 * stripes)(*want_masks)
        _check(self._lib.hec_reconstruct_device_mixed(self._h, _pp(shard_ptrs), _sp(shard_strides),
                                                      _pp([p or 0 for p in out_ptrs]), _sp(out_strides), masks,
                                                      wants, cell_len, stripes, ctypes.c_void_p(workspace_ptr),
                                                      workspace_bytes, ctypes.c_void_p(stream)))

    def reconstruct_crc_device(self, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len, stripes, sums_ptr,
                               want=None, expected_ptr=None, bad_ptr=None, bytes_per_checksum: int = 512,
                               checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_reconstruct_crc_device: reconstruct_device with the rebuilt
        units' chunk sums written to sums_ptr ([stripe][k+m][nck] big-endian
        u32, at the targets' slots) and, with expected_ptr (same layout; may be
        sums_ptr) and bad_ptr ([stripe][k+m] flags, zeroed by the caller), the
        survivors' sums verified in the same pass."""
        _check(self._lib.hec_reconstruct_crc_device(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                    _sp(shard_strides), _pp([p or 0 for p in out_ptrs]),
                                                    _sp(out_strides), _want_bytes(len(shard_ptrs), want), cell_len,
                                                    stripes, bytes_per_checksum, ctypes.c_void_p(expected_ptr),
                                                    ctypes.c_void_p(bad_ptr), ctypes.c_void_p(sums_ptr),
                                                    ctypes.c_void_p(stream)))

    def reconstruct_crc_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_reconstruct_crc_mixed_workspace_size(self._h, stripes)

    def reconstruct_crc_device_mixed(self, shard_ptrs, shard_strides, out_ptrs, out_strides, present_masks,
                                     want_masks, cell_len, stripes, sums_ptr, workspace_ptr, workspace_bytes,
                                     expected_ptr=None, bad_ptr=None, bytes_per_checksum: int = 512,
                                     checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_reconstruct_crc_device_mixed: reconstruct_device_mixed with the
        checksum buffers of reconstruct_crc_device; the workspace is
        reconstruct_crc_mixed_workspace_size(stripes) bytes."""
        masks = (ctypes.c_uint64 * stripes)(*present_masks)
        wants = None if want_masks is None else (ctypes.c_uint64 * stripes)(*want_masks)
        _check(self._lib.hec_reconstruct_crc_device_mixed(self._h, checksum_type, _pp(shard_ptrs), _sp(shard_strides),
                                                          _pp([p or 0 for p in out_ptrs]), _sp(out_strides), masks,
                                                          wants, cell_len, stripes, bytes_per_checksum,
                                                          ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
                                                          ctypes.c_void_p(sums_ptr), ctypes.c_void_p(workspace_ptr),
                                                          workspace_bytes, ctypes.c_void_p(stream)))

    def reconstruct_sums_device(self, shard_ptrs, shard_strides, cell_len, stripes, sums_ptr, want=None,
                                data_len: int = 0, expected_ptr=None, bad_ptr=None, bytes_per_checksum: int = 512,
                                checksum_type: int = CHECKSUM_CRC32C, stream: int = 0) -> None:
        """hec_reconstruct_sums_device: the chunk sums of the lost units
        (shard_ptrs[i] None / 0), reconstructed from the survivors, written to
        their slots of sums_ptr; no cell byte is written.  data_len as for
        composite_crc (0 = every stripe full); expected_ptr / bad_ptr as for
        reconstruct_crc_device."""
        _check(self._lib.hec_reconstruct_sums_device(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                     _sp(shard_strides), _want_bytes(len(shard_ptrs), want), cell_len,
                                                     stripes, bytes_per_checksum, data_len,
                                                     ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
                                                     ctypes.c_void_p(sums_ptr), ctypes.c_void_p(stream)))

    def reconstruct_sums_device_mixed(self, shard_ptrs, shard_strides, present_masks, want_masks, cell_len, stripes,
                                      sums_ptr, workspace_ptr, workspace_bytes, expected_ptr=None, bad_ptr=None,
                                      bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                                      stream: int = 0) -> None:
        """hec_reconstruct_sums_device_mixed: one (present, want) pattern per
        stripe, full stripes only; shard_ptrs[i] may be None / 0 for a unit no
        stripe has present.  The workspace is
        reconstruct_crc_mixed_workspace_size(stripes) bytes."""
        masks = (ctypes.c_uint64 * stripes)(*present_masks)
        wants = None if want_masks is None else (ctypes.c_uint64 * stripes)(*want_masks)
        _check(self._lib.hec_reconstruct_sums_device_mixed(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                           _sp(shard_strides), masks, wants, cell_len, stripes,
                                                           bytes_per_checksum, ctypes.c_void_p(expected_ptr),
                                                           ctypes.c_void_p(bad_ptr), ctypes.c_void_p(sums_ptr),
                                                           ctypes.c_void_p(workspace_ptr), workspace_bytes,
                                                           ctypes.c_void_p(stream)))

    def reconstruct_crc_rows_device(self, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len, stripes,
                                    sums_ptr, want=None, data_len: int = 0, expected_ptr=None, bad_ptr=None,
                                    bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                                    stream: int = 0) -> None:
        """hec_reconstruct_crc_rows_device: reconstruct_crc_device for a group
        whose last stripe is short.  data_len as for composite_crc (0 = every
        stripe full): in the last stripe every unit is verified, rebuilt and
        summed over its own bytes, a rebuilt slot is zero from there up to n0
        and nothing at or past n0 is written."""
        _check(self._lib.hec_reconstruct_crc_rows_device(self._h, checksum_type, _pp([p or 0 for p in shard_ptrs]),
                                                         _sp(shard_strides), _pp([p or 0 for p in out_ptrs]),
                                                         _sp(out_strides), _want_bytes(len(shard_ptrs), want),
                                                         cell_len, stripes, bytes_per_checksum, data_len,
                                                         ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr),
                                                         ctypes.c_void_p(sums_ptr), ctypes.c_void_p(stream)))

    def reconstruct_crc_rows_mixed_workspace_size(self, stripes: int) -> int:
        return self._lib.hec_reconstruct_crc_rows_mixed_workspace_size(self._h, stripes)

    def reconstruct_crc_rows_device_mixed(self, shard_ptrs, shard_strides, out_ptrs, out_strides, present_masks,
                                          want_masks, stripe_bytes, cell_len, stripes, sums_ptr, workspace_ptr,
                                          workspace_bytes, expected_ptr=None, bad_ptr=None,
                                          bytes_per_checksum: int = 512, checksum_type: int = CHECKSUM_CRC32C,
                                          stream: int = 0) -> None:
        """hec_reconstruct_crc_rows_device_mixed: reconstruct_crc_device_mixed
        with the logical bytes of every stripe (stripe_bytes[s]; None = all
        full; 0 or k * cell_len = that stripe is full).  The workspace is
        reconstruct_crc_rows_mixed_workspace_size(stripes) bytes, 8-byte
        aligned."""
        masks = (ctypes.c_uint64 * stripes)(*present_masks)
        wants = None if want_masks is None else (ctypes.c_uint64 * stripes)(*want_masks)
        lens = None if stripe_bytes is None else (ctypes.c_uint64 * stripes)(*stripe_bytes)
        _check(self._lib.hec_reconstruct_crc_rows_device_mixed(
            self._h, checksum_type, _pp(shard_ptrs), _sp(shard_strides), _pp([p or 0 for p in out_ptrs]),
            _sp(out_strides), masks, wants, lens, cell_len, stripes, bytes_per_checksum,
            ctypes.c_void_p(expected_ptr), ctypes.c_void_p(bad_ptr), ctypes.c_void_p(sums_ptr),
            ctypes.c_void_p(workspace_ptr), workspace_bytes, ctypes.c_void_p(stream)))

    def gf_matmul_device(self, matrix: List[List[int]], in_ptrs, in_strides, out_ptrs, out_strides, cell_len,
                         stripes, stream: int = 0) -> None:
        rows, cols = len(matrix), len(matrix[0])
        mat = (ctypes.c_uint8 * (rows * cols))(*[v for r in matrix for v in r])
        _check(self._lib.hec_gf_matmul_device(self._h, mat, rows, cols, _pp(in_ptrs), _sp(in_strides), _pp(out_ptrs),
                                        _sp(out_strides), cell_len, stripes, ctypes.c_void_p(stream)))

    def decode_host_batch(self, vertical_addrs, cell_len: int, rows: int, h_file_addr: int, chunk_rows: int) -> None:
        """vertical_addrs[k+m]: host addresses of the per-shard vertical
        buffers (0/None = missing) -> file-order bytes at h_file_addr."""
        _check(self._lib.hec_decode_host_batch(self._h, _pp([a or 0 for a in vertical_addrs]), cell_len, rows,
                                         ctypes.c_void_p(h_file_addr), chunk_rows))

    def encode_host_batch(self, h_data_addr: int, h_parity_addr: int, cell_len: int, stripes: int,
                          chunk_stripes: int) -> None:
        _check(self._lib.hec_encode_host_batch(self._h, ctypes.c_void_p(h_data_addr), ctypes.c_void_p(h_parity_addr),
                                         cell_len, stripes, chunk_stripes))

    # -- whole files: the last row may be short (CellBuffer semantics) --------
    def encode_rows_host(self, h_data_addr: int, data_len: int, h_parity_addr: int, cell_len: int,
                         chunk_stripes: int = 16) -> None:
        _check(self._lib.hec_encode_rows_host(self._h, ctypes.c_void_p(h_data_addr), data_len,
                                              ctypes.c_void_p(h_parity_addr), cell_len, chunk_stripes))

    def encode_rows_workspace_size(self, cell_len: int) -> int:
        return self._lib.hec_encode_rows_workspace_size(self._h, cell_len)

    def encode_rows_device(self, d_data: int, data_len: int, d_parity: int, cell_len: int, workspace: int,
                           workspace_bytes: int, stream: int = 0) -> None:
        _check(self._lib.hec_encode_rows_device(self._h, ctypes.c_void_p(d_data), data_len, ctypes.c_void_p(d_parity),
                                                cell_len, ctypes.c_void_p(workspace), workspace_bytes,
                                                ctypes.c_void_p(stream)))

    def decode_rows_host(self, vertical_addrs, vertical_lens, cell_len: int, h_file_addr: int, file_len: int,
                         chunk_rows: int = 16) -> None:
        _check(self._lib.hec_decode_rows_host(self._h, _pp([a or 0 for a in vertical_addrs]), _sp(vertical_lens),
                                              cell_len, ctypes.c_void_p(h_file_addr), file_len, chunk_rows))


# ---- torch helpers (device memory comes from torch; plumbing only) --------

def jit_warm(k: int, m: int, missing: Sequence[int], checksum_type: int = 2) -> None:
    """hec_jit_warm: the specialised decode + verify kernel for this plan into
    the code-object caches (no device needed)."""
    present = (ctypes.c_uint8 * (k + m))(*[0 if i in set(missing) else 1 for i in range(k + m)])
    _check(lib.hec_jit_warm(k, m, present, checksum_type))


def jit_stats() -> dict:
    """hec_jit_stats: process totals of the plan-time JIT."""
    v = [ctypes.c_uint64(0) for _ in range(4)]
    lib.hec_jit_stats(*[ctypes.byref(x) for x in v])
    return dict(zip(("compiled", "from_disk", "failed", "launches"), (x.value for x in v)))


def queue_stats(device: int = 0) -> dict:
    """hec_queue_stats: the work-queue counter sets of `device` (streams that
    launched a queue kernel, graph sets handed out to captured launches, and
    whether streams are told apart by hipStreamGetId or by handle)."""
    v = [ctypes.c_uint64(0) for _ in range(2)]
    by_id = ctypes.c_int(0)
    lib.hec_queue_stats(device, *[ctypes.byref(x) for x in v], ctypes.byref(by_id))
    return {"streams": v[0].value, "graph_sets": v[1].value, "keyed_by_id": bool(by_id.value)}


def stripe_layout_ptrs(t, units: int):
    """For a uint8 tensor [stripes, units, cell] return (ptrs, strides)."""
    assert t.dim() == 3 and t.shape[1] == units and t.is_contiguous()
    cell = t.shape[2]
    base = t.data_ptr()
    return [base + i * cell for i in range(units)], [units * cell] * units


def encode_batch(coder: Coder, data, parity, stream=None) -> None:
    """data: uint8 cuda tensor [S, k, cell]; parity: [S, m, cell]."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(data.device)
    dp, ds = stripe_layout_ptrs(data, coder.data_units)
    pp, ps = stripe_layout_ptrs(parity, coder.parity_units)
    coder.encode_device(dp, ds, pp, ps, data.shape[2], data.shape[0], s.cuda_stream)


def crc32c_batch(coder: Coder, cells, bytes_per_checksum: int = 512, stream=None):
    """cells: uint8 cuda tensor [S, n, cell] -> uint8 tensor [S, n, nchunks, 4]
    of big-endian CRC32C per chunk (WritePacket::calculate_checksum)."""
    import torch
    S, n, cell = cells.shape
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    nchunks = (cell + bytes_per_checksum - 1) // bytes_per_checksum
    out = torch.empty((S, n, nchunks, 4), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.crc32c_device(ptrs, strides, cell, S, bytes_per_checksum, out.data_ptr(), s.cuda_stream)
    return out


def checksum_batch(coder: Coder, cells, checksum_type: int = CHECKSUM_CRC32C, bytes_per_checksum: int = 512,
                   stream=None):
    """cells: uint8 cuda tensor [S, n, cell] -> uint8 tensor [S, n, nchunks, 4]
    of big-endian chunk checksums (CRC32C or CRC32 = CRC_32_CKSUM)."""
    import torch
    S, n, cell = cells.shape
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    nchunks = (cell + bytes_per_checksum - 1) // bytes_per_checksum
    out = torch.empty((S, n, nchunks, 4), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.checksum_device(checksum_type, ptrs, strides, cell, S, bytes_per_checksum, out.data_ptr(), s.cuda_stream)
    return out


def composite_crc_batch(coder: Coder, sums, data_units: int, cell_len: int, checksum_type: int = CHECKSUM_CRC32C,
                        bytes_per_checksum: int = 512, data_len: int = 0, want=("cell", "unit", "group"),
                        stream=None, workspace=None):
    """sums: uint8 cuda tensor [S, n, nchunks, 4] as checksum_batch returns ->
    (cell_crcs [S, n, 4], unit_crcs [n, 4], group_crc [4]) uint8 tensors of
    big-endian CRCs, None for an output not in `want`.  Asynchronous on the
    stream; the workspace is allocated here unless one is passed."""
    import torch
    S, n = sums.shape[0], sums.shape[1]
    assert sums.is_contiguous() and sums.shape[2] == (cell_len + bytes_per_checksum - 1) // bytes_per_checksum
    s = stream if stream is not None else torch.cuda.current_stream(sums.device)

    def out(*shape):
        return torch.empty(shape, dtype=torch.uint8, device=sums.device)

    cell = out(S, n, 4) if "cell" in want else None
    unit = out(n, 4) if "unit" in want else None
    group = out(4) if "group" in want else None
    if workspace is None and (unit is not None or group is not None):
        workspace = out(max(4, composite_crc_workspace_size(n, S)))
    coder.composite_crc_device(checksum_type, sums.data_ptr(), n, data_units, cell_len, S, bytes_per_checksum, data_len,
                               cell.data_ptr() if cell is not None else 0, unit.data_ptr() if unit is not None else 0,
                               group.data_ptr() if group is not None else 0,
                               workspace.data_ptr() if workspace is not None else 0,
                               workspace.numel() if workspace is not None else 0, s.cuda_stream)
    if workspace is not None:
        workspace.record_stream(s)
    return cell, unit, group


def checksum_verify_batch(coder: Coder, cells, expected, checksum_type: int = CHECKSUM_CRC32C,
                          bytes_per_checksum: int = 512, stream=None):
    """ReadPacket::get_data's check: -> uint8 tensor [S, n], 1 where a cell
    has a chunk whose checksum differs from `expected` [S, n, nchunks, 4]."""
    import torch
    S, n, cell = cells.shape
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    bad = torch.zeros((S, n), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.checksum_verify_device(checksum_type, ptrs, strides, cell, S, bytes_per_checksum,
                                 expected.data_ptr(), bad.data_ptr(), s.cuda_stream)
    return bad


def decode_verify_batch(coder: Coder, data, parity, missing: Sequence[int], sums, out,
                        checksum_type: int = CHECKSUM_CRC32C, bytes_per_checksum: int = 512, stream=None,
                        missing_parity: Sequence[int] = ()):
    """Verified striped read over data [S,k,cell] / parity [S,m,cell] with
    data shards `missing` (and parity shards `missing_parity`) unavailable
    for the batch; sums [S, k+m, nchunks, 4] are the packets' checksums.
    Rebuilt data lands in out [S,k,cell]; returns the bad-cell flags
    [S, k+m] (uint8 cuda tensor)."""
    import torch
    k, m = coder.data_units, coder.parity_units
    S = data.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(data.device)
    dp, ds = stripe_layout_ptrs(data, k)
    pp, ps = stripe_layout_ptrs(parity, m)
    op, os_ = stripe_layout_ptrs(out, k)
    miss, pmiss = set(missing), set(missing_parity)
    ptrs = [None if i in miss else dp[i] for i in range(k)] + [None if j in pmiss else pp[j] for j in range(m)]
    bad = torch.empty((S, k + m), dtype=torch.uint8, device=data.device)
    coder.decode_verify_device(checksum_type, ptrs, ds + ps, op, os_, data.shape[2], S, bytes_per_checksum,
                               sums.data_ptr(), bad.data_ptr(), s.cuda_stream)
    return bad


def decode_batch_mixed(coder: Coder, data, parity, present_masks: Sequence[int], out, stream=None,
                       workspace=None) -> None:
    """Per-stripe erasure patterns: present_masks[s] bit i = shard i present.
    Rebuilt data shards land in out [S,k,cell] where missing."""
    import torch
    k, m = coder.data_units, coder.parity_units
    S = data.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(data.device)
    dp, ds = stripe_layout_ptrs(data, k)
    pp, ps = stripe_layout_ptrs(parity, m)
    op, os_ = stripe_layout_ptrs(out, k)
    nbytes = coder.decode_mixed_workspace_size(S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=data.device)
    coder.decode_device_mixed(dp + pp, ds + ps, op, os_, list(present_masks), data.shape[2], S,
                              workspace.data_ptr(), workspace.numel(), s.cuda_stream)
    return workspace


def reconstruct_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], want_masks=None, stream=None,
                            workspace=None):
    """Repair in place: cells is a uint8 cuda tensor [S, k+m, cell] holding
    every unit of every stripe; present_masks[s] bit i = unit i of stripe s is
    intact.  The lost units (or those in want_masks[s]) are rebuilt into their
    own slots, data and parity alike.  Returns the workspace (reusable once
    the stream has passed the call)."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    nbytes = coder.reconstruct_mixed_workspace_size(S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=cells.device)
    coder.reconstruct_device_mixed(ptrs, strides, ptrs, strides, list(present_masks),
                                   None if want_masks is None else list(want_masks), cells.shape[2], S,
                                   workspace.data_ptr(), workspace.numel(), s.cuda_stream)
    return workspace


def reconstruct_crc_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], sums, want_masks=None,
                                expected=None, bad=None, checksum_type: int = CHECKSUM_CRC32C, stream=None,
                                workspace=None):
    """reconstruct_batch_mixed with the chunk checksums in the same pass:
    sums is a cuda tensor of S * (k+m) * ceil(cell / 512) 4-byte words (int32
    or 4 uint8 each; big-endian sums) that receives the rebuilt units' chunk
    sums at their own slots; expected (same layout, may be `sums` itself) and
    bad (uint8 [S, k+m], zeroed by the caller) make the call verify the
    survivors every stripe's plan reads, flagging a mismatch in bad.  Returns
    the workspace (reusable once the stream has passed the call)."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    nbytes = coder.reconstruct_crc_mixed_workspace_size(S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=cells.device)
    coder.reconstruct_crc_device_mixed(ptrs, strides, ptrs, strides, list(present_masks),
                                       None if want_masks is None else list(want_masks), cells.shape[2], S,
                                       sums.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       expected_ptr=None if expected is None else expected.data_ptr(),
                                       bad_ptr=None if bad is None else bad.data_ptr(),
                                       checksum_type=checksum_type, stream=s.cuda_stream)
    return workspace


def reconstruct_crc_rows_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], sums, stripe_bytes=None,
                                     want_masks=None, expected=None, bad=None, checksum_type: int = CHECKSUM_CRC32C,
                                     bytes_per_checksum: int = 512, stream=None, workspace=None):
    """reconstruct_crc_batch_mixed for a batch with short stripes:
    stripe_bytes[s] = the logical bytes of stripe s (None = all full; 0 or
    k * cell = that stripe is full).  In a short stripe every unit is verified,
    rebuilt and summed over its own bytes, a rebuilt slot is zero from its
    length up to n0 = min(cell, stripe_bytes[s]) and nothing at or past n0 is
    written.  Returns the workspace (reusable once the stream has passed the
    call)."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    nbytes = coder.reconstruct_crc_rows_mixed_workspace_size(S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=cells.device)
    coder.reconstruct_crc_rows_device_mixed(ptrs, strides, ptrs, strides, list(present_masks),
                                            None if want_masks is None else list(want_masks),
                                            None if stripe_bytes is None else list(stripe_bytes), cells.shape[2], S,
                                            sums.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                            expected_ptr=None if expected is None else expected.data_ptr(),
                                            bad_ptr=None if bad is None else bad.data_ptr(),
                                            bytes_per_checksum=bytes_per_checksum, checksum_type=checksum_type,
                                            stream=s.cuda_stream)
    return workspace


def encode_crc_rows_batch(coder: Coder, cells, sums, data_len: int = 0, stripe_bytes=None,
                          checksum_type: int = CHECKSUM_CRC32C, bytes_per_checksum: int = 512, stream=None,
                          workspace=None):
    """Parity and chunk sums of a batch with short stripes: cells is a uint8
    cuda tensor [S, k+m, width] (units 0 .. k-1 are read, k .. k+m-1 written),
    sums the [S, k+m, nck] sums array.  With stripe_bytes (one entry per stripe;
    0 or k * width = that stripe is full) the mixed form runs, else the uniform
    form with data_len (0 = every stripe full).  A short stripe's parity units
    get their n0 bytes and nothing behind, and every unit the sums of its own
    bytes.  Returns the workspace the mixed form allocated or was given
    (reusable once the stream has passed the call), or None."""
    import torch
    k, m = coder.data_units, coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, k + m)
    if stripe_bytes is None:
        coder.encode_crc_rows_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], cells.shape[2], S, sums.data_ptr(),
                                     data_len=data_len, bytes_per_checksum=bytes_per_checksum,
                                     checksum_type=checksum_type, stream=s.cuda_stream)
        return None
    if data_len:
        raise ValueError("encode_crc_rows_batch: data_len or stripe_bytes, not both")
    if workspace is None:
        workspace = torch.empty(max(coder.encode_crc_rows_mixed_workspace_size(S), 8), dtype=torch.uint8,
                                device=cells.device)
        workspace.record_stream(s)
    coder.encode_crc_rows_device_mixed(ptrs[:k], strides[:k], ptrs[k:], strides[k:], list(stripe_bytes),
                                       cells.shape[2], S, sums.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                       bytes_per_checksum=bytes_per_checksum, checksum_type=checksum_type,
                                       stream=s.cuda_stream)
    return workspace


def read_crc_rows_batch(coder: Coder, cells, present_masks: Sequence[int], expected, file, data_len: int = 0,
                        stripe_bytes=None, bad=None, file_stride: int = 0, checksum_type: int = CHECKSUM_CRC32C,
                        bytes_per_checksum: int = 512, stream=None, workspace=None):
    """The verified striped read of a batch into file order: cells is a uint8
    cuda tensor [S, k+m, width], present_masks[s] the units stripe s has,
    expected the [S, k+m, nck] sums array (None = no verification), file a
    uint8 cuda tensor that receives data unit u of stripe s at s * file_stride
    + u * width (file_stride 0 = k * width) for its own length, and bad the
    zeroed [S, k+m] flags.  With one mask for all stripes and no stripe_bytes
    the uniform form runs with data_len (0 = every stripe full), else the mixed
    form with stripe_bytes (0 or k * width = that stripe is full).  Nothing at
    or past a stripe's logical end is written.  Returns the workspace the mixed
    form allocated or was given (reusable once the stream has passed the
    call), or None."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    kw = dict(file_stride=file_stride, expected_ptr=None if expected is None else expected.data_ptr(),
              bad_ptr=None if bad is None else bad.data_ptr(), bytes_per_checksum=bytes_per_checksum,
              checksum_type=checksum_type, stream=s.cuda_stream)
    masks = list(present_masks)
    if stripe_bytes is None and len(set(masks)) <= 1:
        mask = masks[0] if masks else (1 << n) - 1
        coder.read_crc_rows_device([p if (mask >> i) & 1 else None for i, p in enumerate(ptrs)], strides,
                                   file.data_ptr(), cells.shape[2], S, data_len=data_len, **kw)
        return None
    if data_len and stripe_bytes is not None:
        raise ValueError("read_crc_rows_batch: data_len or stripe_bytes, not both")
    if data_len:  # several masks: the last stripe's length goes into the mixed form
        full = coder.data_units * cells.shape[2]
        last = data_len - (S - 1) * full
        if not 0 < last <= full:
            raise ValueError("read_crc_rows_batch: data_len does not end in the last stripe")
        stripe_bytes = [0] * (S - 1) + [last]
    if workspace is None:
        workspace = torch.empty(max(coder.read_crc_rows_mixed_workspace_size(S), 8), dtype=torch.uint8,
                                device=cells.device)
        workspace.record_stream(s)
    coder.read_crc_rows_device_mixed(ptrs, strides, file.data_ptr(), masks,
                                     None if stripe_bytes is None else list(stripe_bytes), cells.shape[2], S,
                                     workspace.data_ptr(), workspace.numel(), **kw)
    return workspace


def reconstruct_sums_batch(coder: Coder, cells, present_masks: Sequence[int], sums, want_masks=None, expected=None,
                           bad=None, checksum_type: int = CHECKSUM_CRC32C, bytes_per_checksum: int = 512,
                           stream=None, workspace=None):
    """The chunk sums of the lost units of a batch, nothing rebuilt written:
    cells, present_masks, sums, expected and bad as for
    reconstruct_crc_batch_mixed, but cells is only read -- the slots of lost
    units are never touched -- and sums receives the sums of the lost units
    (or those in want_masks[s]) at their own slots.  A unit no stripe has
    present is passed without storage.  Returns the workspace (reusable once
    the stream has passed the call)."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    ever = 0
    for mask in present_masks:
        ever |= mask
    ptrs = [p if (ever >> i) & 1 else None for i, p in enumerate(ptrs)]
    nbytes = coder.reconstruct_crc_mixed_workspace_size(S)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=cells.device)
    coder.reconstruct_sums_device_mixed(ptrs, strides, list(present_masks),
                                        None if want_masks is None else list(want_masks), cells.shape[2], S,
                                        sums.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                        expected_ptr=None if expected is None else expected.data_ptr(),
                                        bad_ptr=None if bad is None else bad.data_ptr(),
                                        bytes_per_checksum=bytes_per_checksum, checksum_type=checksum_type,
                                        stream=s.cuda_stream)
    return workspace


def scrub_batch(coder: Coder, cells, stream=None):
    """Scrub every stripe of cells, a uint8 cuda tensor [S, k+m, cell] (the
    layout reconstruct_batch_mixed takes): -> int64 cuda tensor [S, 2] of
    (ruled_out, bad_bytes) per stripe, (0, 0) where the stripe is consistent.
    Read-only over cells; asynchronous on the stream."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    out = torch.empty((S, 2), dtype=torch.int64, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.scrub_device(ptrs, strides, cells.shape[2], S, out.data_ptr(), s.cuda_stream)
    return out


def scrub_correct_batch(coder: Coder, cells, results, units=None, stream=None):
    """Fix, in place, the unit that a scrub located in each stripe of cells
    (uint8 cuda tensor [S, k+m, cell]): results is the int64 [S, 2] tensor
    scrub_batch or scrub_crc_batch returned for these very cells on the same
    stream, with no write to cells in between.  -> int32 cuda tensor [S]: the
    corrected unit, CORRECT_CLEAN or CORRECT_UNLOCATED (stripe untouched).
    Pass `units` to write into a tensor of your own.  One kernel, no workspace;
    asynchronous on the stream."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    if units is None:
        with torch.cuda.stream(s):
            units = torch.empty((S,), dtype=torch.int32, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.scrub_correct_device(ptrs, strides, cells.shape[2], S, results.data_ptr(), units.data_ptr(), s.cuda_stream)
    return units


def scrub_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], stream=None, workspace=None):
    """scrub_batch for degraded stripes: present_masks[s] bit i = unit i of
    stripe s is there (the other slots of cells are not read).  -> int64 cuda
    tensor [S, 2]; a stripe with k units or fewer gives (0, 0) unchecked, a bad
    stripe has its missing units' bits set in ruled_out (scrub_verdict works
    unchanged).  Pass `workspace` (uint8 cuda tensor of
    coder.scrub_mixed_workspace_size(S) bytes) to reuse one; it must stay
    untouched until the stream has passed the call."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    out = torch.empty((S, 2), dtype=torch.int64, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    if workspace is None:
        workspace = torch.empty(max(coder.scrub_mixed_workspace_size(S), 1), dtype=torch.uint8, device=cells.device)
        workspace.record_stream(s)
    coder.scrub_device_mixed(ptrs, strides, list(present_masks), cells.shape[2], S, out.data_ptr(),
                             workspace.data_ptr(), workspace.numel(), s.cuda_stream)
    return out


def scrub_crc_batch(coder: Coder, cells, expected, bad=None, checksum_type: int = CHECKSUM_CRC32C, stream=None):
    """scrub_batch with the chunk checksums in the same pass: expected is a
    cuda tensor of S * (k+m) * ceil(cell / 512) 4-byte words (int32 or 4 uint8
    each; big-endian sums) that every unit is verified against.  -> (results,
    bad): the int64 [S, 2] tensor of scrub_batch and the uint8 [S, k+m] flags
    (1 = the unit does not match its sums).  Pass `bad` to accumulate into a
    tensor of your own (flags are only ever set); otherwise a zeroed one is
    made.  Read-only over cells and expected; asynchronous on the stream."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    with torch.cuda.stream(s):
        out = torch.empty((S, 2), dtype=torch.int64, device=cells.device)
        if bad is None:
            bad = torch.zeros((S, n), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    coder.scrub_crc_device(ptrs, strides, cells.shape[2], S, expected.data_ptr(), bad.data_ptr(), out.data_ptr(),
                           checksum_type=checksum_type, stream=s.cuda_stream)
    return out, bad


def scrub_crc_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], expected, bad=None,
                          checksum_type: int = CHECKSUM_CRC32C, stream=None, workspace=None):
    """scrub_crc_batch for degraded stripes: present_masks[s] bit i = unit i of
    stripe s is there (the other slots of cells and expected are not read).
    -> (results, bad) as scrub_crc_batch, results as scrub_batch_mixed; the
    present units of a stripe with k units or fewer are still verified.  Pass
    `workspace` (uint8 cuda tensor of coder.scrub_crc_mixed_workspace_size(S)
    bytes) to reuse one; it must stay untouched until the stream has passed
    the call."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    with torch.cuda.stream(s):
        out = torch.empty((S, 2), dtype=torch.int64, device=cells.device)
        if bad is None:
            bad = torch.zeros((S, n), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    if workspace is None:
        workspace = torch.empty(max(coder.scrub_crc_mixed_workspace_size(S), 1), dtype=torch.uint8,
                                device=cells.device)
        workspace.record_stream(s)
    coder.scrub_crc_device_mixed(ptrs, strides, list(present_masks), cells.shape[2], S, expected.data_ptr(),
                                 bad.data_ptr(), out.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                 checksum_type=checksum_type, stream=s.cuda_stream)
    return out, bad


def scrub_crc_rows_batch_mixed(coder: Coder, cells, present_masks: Sequence[int], expected, stripe_bytes=None,
                               bad=None, checksum_type: int = CHECKSUM_CRC32C, bytes_per_checksum: int = 512,
                               stream=None, workspace=None):
    """scrub_crc_batch_mixed for a batch with short stripes: stripe_bytes[s] =
    the logical bytes of stripe s (None = all full; 0 or k * cell = that stripe
    is full).  A short stripe is checked over its positions below n0 =
    min(cell, stripe_bytes[s]) with every unit zero from its own length on, and
    every present unit is verified over its own bytes.  -> (results, bad) as
    scrub_crc_batch_mixed.  Pass `workspace` (uint8 cuda tensor of
    coder.scrub_crc_rows_mixed_workspace_size(S) bytes) to reuse one; it must
    stay untouched until the stream has passed the call."""
    import torch
    n = coder.data_units + coder.parity_units
    S = cells.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(cells.device)
    with torch.cuda.stream(s):
        out = torch.empty((S, 2), dtype=torch.int64, device=cells.device)
        if bad is None:
            bad = torch.zeros((S, n), dtype=torch.uint8, device=cells.device)
    ptrs, strides = stripe_layout_ptrs(cells, n)
    if workspace is None:
        workspace = torch.empty(max(coder.scrub_crc_rows_mixed_workspace_size(S), 1), dtype=torch.uint8,
                                device=cells.device)
        workspace.record_stream(s)
    coder.scrub_crc_rows_device_mixed(ptrs, strides, list(present_masks),
                                      None if stripe_bytes is None else list(stripe_bytes), cells.shape[2], S,
                                      expected.data_ptr(), bad.data_ptr(), out.data_ptr(), workspace.data_ptr(),
                                      workspace.numel(), bytes_per_checksum=bytes_per_checksum,
                                      checksum_type=checksum_type, stream=s.cuda_stream)
    return out, bad


def decode_batch(coder: Coder, data, parity, missing: Sequence[int], out, stream=None) -> None:
    """Reconstruct data shards `missing` of every stripe (one erasure pattern
    for the batch) from data [S,k,cell] / parity [S,m,cell] into out
    [S,k,cell] (only the missing slots are written)."""
    import torch
    k, m = coder.data_units, coder.parity_units
    s = stream if stream is not None else torch.cuda.current_stream(data.device)
    dp, ds = stripe_layout_ptrs(data, k)
    pp, ps = stripe_layout_ptrs(parity, m)
    op, os_ = stripe_layout_ptrs(out, k)
    miss = set(missing)
    ptrs = [None if i in miss else dp[i] for i in range(k)] + pp
    coder.decode_device(ptrs, ds + ps, op, os_, data.shape[2], data.shape[0], s.cuda_stream)


class _Borrowed(Coder):
    """A group slot's coder: the group owns (and destroys) the handle."""

    def __init__(self, handle, k, m, device, codec):  # noqa: D107 (no super().__init__: no new coder)
        self._lib = lib
        self._h = handle
        self.codec, self.data_units, self.parity_units, self.device = codec, k, m, device

    def close(self) -> None:
        self._h = None


class CoderGroup:
    """Multi-GPU coder group (hec_group_*): a batch split into
    contiguous stripe ranges, one per device, each on its own host thread."""

    def __init__(self, data_units: int, parity_units: int, devices: Sequence[int], codec: str = "rs"):
        h = ctypes.c_void_p()
        devs = (ctypes.c_int * len(devices))(*devices)
        _check(lib.hec_group_create(codec.encode(), data_units, parity_units, devs, len(devices), ctypes.byref(h)))
        self._h = h
        self.data_units, self.parity_units, self.devices, self.codec = data_units, parity_units, list(devices), codec

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib.hec_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return lib.hec_group_size(self._h)

    def coder(self, slot: int) -> Coder:
        h = lib.hec_group_coder(self._h, slot)
        if not h:
            raise IndexError(slot)
        return _Borrowed(ctypes.c_void_p(h), self.data_units, self.parity_units, self.devices[slot], self.codec)

    def range(self, total: int, slot: int):
        first, count = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib.hec_group_range(self._h, total, slot, ctypes.byref(first), ctypes.byref(count)))
        return first.value, count.value

    def encode_host_batch(self, h_data_addr: int, h_parity_addr: int, cell_len: int, stripes: int,
                          chunk_stripes: int) -> None:
        _check(lib.hec_group_encode_host_batch(self._h, ctypes.c_void_p(h_data_addr), ctypes.c_void_p(h_parity_addr),
                                               cell_len, stripes, chunk_stripes))

    def decode_host_batch(self, vertical_addrs, cell_len: int, rows: int, h_file_addr: int, chunk_rows: int) -> None:
        _check(lib.hec_group_decode_host_batch(self._h, _pp([a or 0 for a in vertical_addrs]), cell_len, rows,
                                               ctypes.c_void_p(h_file_addr), chunk_rows))

    def encode_device(self, data_ptrs, data_strides, parity_ptrs, parity_strides, cell_len: int, stripes,
                      streams=None) -> None:
        """hec_group_encode_device: per-slot lists (slot-major), each slot's
        stripes on its own device; asynchronous on `streams` (raw handles)."""
        _check(lib.hec_group_encode_device(self._h, _pp(data_ptrs), _sp(data_strides), _pp(parity_ptrs),
                                           _sp(parity_strides), cell_len, _sp(stripes),
                                           _pp(streams) if streams is not None else None))

    def decode_device(self, shard_ptrs, shard_strides, out_ptrs, out_strides, cell_len: int, stripes,
                      streams=None) -> None:
        """hec_group_decode_device: shard_ptrs slot-major k+m per slot (None =
        missing), out_ptrs k per slot."""
        _check(lib.hec_group_decode_device(self._h, _pp([a or 0 for a in shard_ptrs]), _sp(shard_strides),
                                           _pp([a or 0 for a in out_ptrs]), _sp(out_strides), cell_len,
                                           _sp(stripes), _pp(streams) if streams is not None else None))
