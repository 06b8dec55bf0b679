"""Measurement probe (GPU box): the composite-CRC fold (hec_composite_crc_device,
csrc/crc_compose.hip) against the first step of the only route a caller had
before it, on one MI355X, product library, one process, HIP events around REPS
back-to-back repetitions, rounds alternated.  Per config (CRC32C per 512-B
chunk, all three outputs):
  composite   hec_composite_crc_device over the [S][n][nck] chunk sums;
  copy        the same sums array to pinned host memory (hipMemcpyAsync), after
              which the caller would still have to fold it on a host core;
  checksum    hec_checksum_device over the cells that produce those sums, for scale.
The device result is compared with hec_composite_crc on the same sums before
anything is timed.
  python3 scripts/probe_composite_crc.py
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hdfs_native_ec as H  # noqa: E402

CONFIGS = [(6, 3, 1 << 20, 1024), (10, 4, 1 << 20, 256), (6, 3, 64 << 10, 65536)]
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "5"))
REPS = int(os.environ.get("PROBE_REPS", "8"))
BPC = 512
PEAK = 8e12  # HBM bytes/s


def timed(stream, fn):
    fn()  # warm
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def report(name, variant, ts, nbytes, what):
    med, lo, hi = statistics.median(ts), min(ts), max(ts)
    print(f"{name:24s} {variant:10s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
          f"{nbytes / (med * 1e-3) / 1e9:.1f} GB/s = {nbytes / (med * 1e-3) / PEAK:.4f} of 8 TB/s over {what}",
          flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    for k, m, cell, S in CONFIGS:
        n, nck = k + m, cell // BPC
        name = f"RS({k},{m}) {cell >> 10} KiB x {S}"
        coder = H.Coder(k, m, 0)
        cells = torch.empty((S, n, cell), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=g)
        ptrs, strides = H.stripe_layout_ptrs(cells, n)
        sums = torch.empty((S, n, nck, 4), dtype=torch.uint8, device=dev)
        pinned = torch.empty(sums.shape, dtype=torch.uint8, pin_memory=True)
        cell_crcs = torch.empty((S, n, 4), dtype=torch.uint8, device=dev)
        unit_crcs = torch.empty((n, 4), dtype=torch.uint8, device=dev)
        group_crc = torch.empty((4,), dtype=torch.uint8, device=dev)
        ws = torch.empty(H.composite_crc_workspace_size(n, S), dtype=torch.uint8, device=dev)

        def checksum():
            coder.checksum_device(H.CHECKSUM_CRC32C, ptrs, strides, cell, S, BPC, sums.data_ptr(), st)

        def composite():
            coder.composite_crc_device(H.CHECKSUM_CRC32C, sums.data_ptr(), n, k, cell, S, BPC, 0, cell_crcs.data_ptr(),
                                       unit_crcs.data_ptr(), group_crc.data_ptr(), ws.data_ptr(), ws.numel(), st)

        def copy():
            pinned.copy_(sums, non_blocking=True)

        checksum()
        composite()
        copy()
        torch.cuda.synchronize()
        # the host fold of the copied sums is the check
        host = [np.zeros(4 * S * n, dtype=np.uint8), np.zeros(4 * n, dtype=np.uint8), np.zeros(4, dtype=np.uint8)]
        vp = ctypes.c_void_p
        H._check(H.lib.hec_composite_crc(H.CHECKSUM_CRC32C, vp(pinned.data_ptr()), n, k, cell, S, BPC, 0,
                                         *[vp(h.ctypes.data) for h in host]))
        for h, d in zip(host, (cell_crcs, unit_crcs, group_crc)):
            assert np.array_equal(h, d.cpu().numpy().reshape(-1)), (name, "device and host folds differ")
        t_fold, t_copy, t_sum = [], [], []
        for _ in range(ROUNDS):
            t_fold.append(timed(stream, composite))
            t_copy.append(timed(stream, copy))
            t_sum.append(timed(stream, checksum))
        report(name, "composite", t_fold, sums.numel(), "the sums")
        report(name, "copy", t_copy, sums.numel(), "the sums")
        report(name, "checksum", t_sum, cells.numel(), "the cells")
        bound = statistics.median(t_copy) - (max(t_copy) - min(t_copy))
        med = statistics.median(t_fold)
        print(f"{name:24s} acceptance: composite median {med:.4f} ms vs copy median - spread {bound:.4f} ms: "
              f"{'PASS' if med <= bound else 'FAIL'} ({statistics.median(t_copy) / med:.1f}x)", flush=True)
        coder.close()
        del cells, sums, pinned, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
