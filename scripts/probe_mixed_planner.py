"""Measurement probe (GPU box): the host side of hec_reconstruct_device_mixed.
RS(6,3), 65 536 stripes of 1024 bytes, per stripe 0..3 units lost at random
(every pattern of the code shows up, runs are short; 256 KiB of plan offsets
are past the fused kernel's resident LDS, so the call goes per run of stripes,
one launch each): the host clock around the C call alone -- grouping and
every launch queued, no synchronise inside; the stream is drained between
calls, outside the clock.
The ctypes arguments are built once, so the wrapper's marshalling is not in it.
HEC_LIB_PATH picks the library (profiles/mixed_planner/README.md).
  python3 scripts/probe_mixed_planner.py
"""
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hdfs_native_ec as H  # noqa: E402

K, M, S, CELL = 6, 3, 65536, 1024
CALLS = int(os.environ.get("PROBE_CALLS", "10"))


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    n = K + M
    coder = H.Coder(K, M, 0)
    cells = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
    cells.random_(0, 256)
    ptrs, strides = H.stripe_layout_ptrs(cells, n)
    coder.encode_device(ptrs[:K], strides[:K], ptrs[K:], strides[K:], CELL, S, stream.cuda_stream)
    truth = cells.clone()
    rng = np.random.default_rng(0x5EED_EC63)
    full = (1 << n) - 1
    masks = [full & ~sum(1 << int(i) for i in rng.choice(n, size=int(rng.integers(0, M + 1)), replace=False))
             for _ in range(S)]
    lost = torch.tensor([[not (mk >> j) & 1 for j in range(n)] for mk in masks], device=dev)
    cells[lost] = 0xEE
    ws = torch.empty(coder.reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    pp = (ctypes.c_void_p * n)(*ptrs)
    sp = (ctypes.c_size_t * n)(*strides)
    mk = (ctypes.c_uint64 * S)(*masks)
    args = (coder.handle, pp, sp, pp, sp, mk, None, CELL, S, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
            ctypes.c_void_p(stream.cuda_stream))

    def call():
        t0 = time.perf_counter()
        rc = H.lib.hec_reconstruct_device_mixed(*args)
        t1 = time.perf_counter()
        assert rc == 0, rc
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3

    call()  # warm: code objects, plan cache, pinned staging; repairs the cells
    assert torch.equal(cells, truth)
    ts = [call() for _ in range(CALLS)]  # repairing repaired cells: the same work
    print(f"RS({K},{M}) x {S} x {CELL} B, {len(set(masks))} patterns: host enqueue of reconstruct_device_mixed "
          f"median {statistics.median(ts):.3f} ms  [{min(ts):.3f} .. {max(ts):.3f}]  over {CALLS} calls", flush=True)
    coder.close()


if __name__ == "__main__":
    main()
