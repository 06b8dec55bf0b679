"""Measurement probe (GPU box): verified reconstruction
(hec_reconstruct_crc_device_mixed, kernel gf_reconstruct_crc) against what a
caller composes from the calls that existed before it, on one MI355X, product
library, one process, the same buffers, rounds alternated, HIP events around
REPS back-to-back repetitions.  Per config, RS(6,3) 1 MiB x 1024 and RS(10,4)
1 MiB x 256: one lost unit per stripe, index uniform over k+m (a dead
DataNode's block groups), repaired in place, CRC32C per 512-B chunk.

The yardstick, per repetition (the batch is ordered by lost unit, as a caller
that has to use these calls would order it, so every run of stripes shares
its survivors):
  hec_checksum_verify_device over the k survivors of every run (expected sums
    re-packed per run into the compact [stripe][k] layout that call needs),
  hec_reconstruct_device_mixed over the batch,
  hec_checksum_device over the rebuilt unit of every run (compact output).
Beside it: hec_reconstruct_crc_device_mixed with d_expected (one sums array,
d_expected == d_sums) and without.  Everything is checked against the original
cells and their sums before anything is timed.
  python3 scripts/probe_reconstruct_crc.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hdfs_native_ec as H  # noqa: E402

CELL = int(os.environ.get("PROBE_CELL", str(1 << 20)))
CONFIGS = [(6, 3, 1024), (10, 4, 256)]
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "5"))
REPS = int(os.environ.get("PROBE_REPS", "8"))
BPC = 512
PEAK = 8e12  # HBM bytes/s


def timed(stream, fn):
    fn()  # warm: code objects, plan cache, pinned staging
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def report(name, variant, ts, nbytes):
    med, lo, hi = statistics.median(ts), min(ts), max(ts)
    print(f"{name:16s} {variant:34s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
          f"{nbytes / (med * 1e-3) / PEAK:.3f} of peak over k reads + 1 write", flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    nck = -(-CELL // BPC)
    for k, m, S in CONFIGS:
        n = k + m
        name = f"RS({k},{m}) x {S}"
        coder = H.Coder(k, m, 0)
        cells = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=g)
        ptrs, strides = H.stripe_layout_ptrs(cells, n)
        stride = strides[0]
        coder.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], CELL, S, st)
        # the true sums of every cell, [S][n][nck]
        true = torch.empty((S, n, nck), dtype=torch.int32, device=dev)
        H._check(H.lib.hec_checksum_device(coder.handle, H.CHECKSUM_CRC32C, H._pp(ptrs), H._sp(strides), n, CELL, S,
                                           BPC, true.data_ptr(), st))
        torch.cuda.synchronize()
        rng = np.random.default_rng(0x5EED_EC00 + k)
        full = (1 << n) - 1
        lost_unit = np.sort(rng.integers(0, n, size=S))
        masks = [full & ~(1 << int(u)) for u in lost_unit]
        idx = torch.arange(S, device=dev)
        unit = torch.from_numpy(lost_unit).to(dev)
        saved = cells[idx, unit].clone()
        # runs of stripes sharing a lost unit: (first stripe, count, unit, survivors)
        runs = []
        for u in sorted(set(lost_unit.tolist())):
            where = np.flatnonzero(lost_unit == u)
            surv = [i for i in range(n) if i != u][:k]
            runs.append((int(where[0]), len(where), u, surv))
        # the composition's compact buffers
        exp_c = [true[s0:s0 + cnt][:, surv].contiguous() for (s0, cnt, u, surv) in runs]
        bad_c = torch.zeros((S, k), dtype=torch.uint8, device=dev)
        out_c = torch.zeros((S, nck), dtype=torch.int32, device=dev)
        ws_r = torch.empty(coder.reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        # the fused call's: one sums array in the engine's layout, the lost slots to be filled in
        sums = true.clone()
        bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        ws_f = torch.empty(coder.reconstruct_crc_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

        def scribble():
            cells[idx, unit] = 0xEE
            sums[idx, unit] = 0x5A5A5A5A
            out_c.fill_(0x5A5A5A5A)

        def composed():
            for (s0, cnt, u, surv), e in zip(runs, exp_c):
                H._check(H.lib.hec_checksum_verify_device(
                    coder.handle, H.CHECKSUM_CRC32C, H._pp([ptrs[i] + s0 * stride for i in surv]), H._sp([stride] * k),
                    k, CELL, cnt, BPC, e.data_ptr(), bad_c.data_ptr() + s0 * k, st))
            coder.reconstruct_device_mixed(ptrs, strides, ptrs, strides, masks, None, CELL, S, ws_r.data_ptr(),
                                           ws_r.numel(), st)
            for (s0, cnt, u, surv) in runs:
                H._check(H.lib.hec_checksum_device(
                    coder.handle, H.CHECKSUM_CRC32C, H._pp([ptrs[u] + s0 * stride]), H._sp([stride]), 1, CELL, cnt,
                    BPC, out_c.data_ptr() + s0 * nck * 4, st))

        def fused(verify):
            coder.reconstruct_crc_device_mixed(ptrs, strides, ptrs, strides, masks, None, CELL, S, sums.data_ptr(),
                                               ws_f.data_ptr(), ws_f.numel(),
                                               expected_ptr=sums.data_ptr() if verify else None,
                                               bad_ptr=bad.data_ptr() if verify else None, stream=st)

        for label, fn in (("composition", composed), ("fused + verify", lambda: fused(True)),
                          ("fused", lambda: fused(False))):
            scribble()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(cells[idx, unit], saved), (name, label, "cells")
            if label == "composition":
                assert torch.equal(out_c, true[idx, unit]), (name, label, "sums")
                assert not bool(bad_c.any()), (name, label, "flags")
            else:
                assert torch.equal(sums, true), (name, label, "sums")
                assert not bool(bad.any()), (name, label, "flags")
        t_c, t_v, t_f = [], [], []
        for _ in range(ROUNDS):
            t_c.append(timed(stream, composed))
            t_v.append(timed(stream, lambda: fused(True)))
            t_f.append(timed(stream, lambda: fused(False)))
        nbytes = (k + 1) * S * CELL
        n_par = int((lost_unit >= k).sum())
        print(f"{name}: {len(runs)} runs, {n_par}/{S} parity units lost", flush=True)
        report(name, "verify + reconstruct + checksum", t_c, nbytes)
        report(name, "reconstruct_crc (d_expected)", t_v, nbytes)
        report(name, "reconstruct_crc (no d_expected)", t_f, nbytes)
        bound = statistics.median(t_c) - (max(t_c) - min(t_c))
        for label, ts in (("d_expected", t_v), ("no d_expected", t_f)):
            med = statistics.median(ts)
            print(f"{name:16s} acceptance ({label}): fused median {med:.4f} ms vs composition median - spread "
                  f"{bound:.4f} ms: {'PASS' if med <= bound else 'FAIL'} ({statistics.median(t_c) / med:.2f}x)",
                  flush=True)
        coder.close()
        del cells, saved, true, sums
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
