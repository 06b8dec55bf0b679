"""Measurement probe (GPU box): verified scrub (hec_scrub_crc_device and
hec_scrub_crc_device_mixed, kernel gf_scrub_crc) against what a caller composes
from the calls that existed before it, on one MI355X, product library, one
process, the same buffers, rounds alternated, HIP events around REPS
back-to-back repetitions.  Per config, RS(6,3) 1 MiB x 1024 and RS(10,4)
1 MiB x 256, CRC32C per 512-B chunk, three batches:
  clean        every unit present, nothing wrong;
  1% dirty     every unit present, one byte flipped in 1 % of the stripes (the
               sums left alone: a flag and a located unit each);
  node failure one lost unit per stripe, index uniform over k+m, nothing wrong.

The yardstick, per repetition:
  all present:  hec_checksum_verify_device over the k+m units + hec_scrub_device;
  node failure: the batch ordered by lost unit (as a caller that has to use
    these calls would order it), hec_checksum_verify_device over the k+m-1
    present units of every run (expected sums re-packed per run into the
    compact layout that call needs) + hec_scrub_device_mixed over the batch.
Everything is compared (results, flags) between the two before anything is
timed.
  python3 scripts/probe_scrub_crc.py
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
    print(f"{name:28s} {variant:24s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
          f"{nbytes / (med * 1e-3) / PEAK:.3f} of peak over (k+e) reads", flush=True)
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
        rng = np.random.default_rng(0x5C12_0B00 + k)
        full = (1 << n) - 1
        res_c = torch.empty((S, 2), dtype=torch.int64, device=dev)
        res_f = torch.empty((S, 2), dtype=torch.int64, device=dev)
        bad_c = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        bad_f = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        ws_s = torch.empty(coder.scrub_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        ws_f = torch.empty(coder.scrub_crc_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

        # ---- every unit present: clean, then 1 % dirty --------------------------
        def composed_full():
            coder.checksum_verify_device(H.CHECKSUM_CRC32C, ptrs, strides, CELL, S, BPC, true.data_ptr(),
                                         bad_c.data_ptr(), st)
            coder.scrub_device(ptrs, strides, CELL, S, res_c.data_ptr(), st)

        def fused_full():
            coder.scrub_crc_device(ptrs, strides, CELL, S, true.data_ptr(), bad_f.data_ptr(), res_f.data_ptr(),
                                   stream=st)

        dirty = np.sort(rng.choice(S, size=max(S // 100, 1), replace=False))
        d_unit = rng.integers(0, n, size=len(dirty))
        d_byte = rng.integers(0, CELL, size=len(dirty))
        for batch in ("clean", "1% dirty"):
            name = f"RS({k},{m}) x {S} {batch}"
            if batch != "clean":
                for s, u, b in zip(dirty, d_unit, d_byte):
                    cells[int(s), int(u), int(b)] ^= 0x40
            bad_c.zero_()
            bad_f.zero_()
            composed_full()
            fused_full()
            torch.cuda.synchronize()
            assert torch.equal(res_c, res_f), (name, "results")
            assert torch.equal(bad_c, bad_f), (name, "flags")
            want = 0 if batch == "clean" else len(dirty)
            assert int((res_f[:, 1] != 0).sum()) == want and int(bad_f.sum()) == want, (name, "dirty stripes")
            t_c, t_f = [], []
            for _ in range(ROUNDS):
                t_c.append(timed(stream, composed_full))
                t_f.append(timed(stream, fused_full))
            nbytes = n * S * CELL
            report(name, "verify + scrub", t_c, nbytes)
            report(name, "scrub_crc", t_f, nbytes)
            accept(name, t_c, t_f)
        for s, u, b in zip(dirty, d_unit, d_byte):  # clean again
            cells[int(s), int(u), int(b)] ^= 0x40

        # ---- after one node failure ------------------------------------------------
        name = f"RS({k},{m}) x {S} node failure"
        lost_unit = np.sort(rng.integers(0, n, size=S))
        masks = [full & ~(1 << int(u)) for u in lost_unit]
        # the lost slots hold bytes that match nothing
        idx = torch.arange(S, device=dev)
        cells[idx, torch.from_numpy(lost_unit).to(dev)] = 0xEE
        runs = []  # (first stripe, count, lost unit, present units)
        for u in sorted(set(lost_unit.tolist())):
            where = np.flatnonzero(lost_unit == u)
            runs.append((int(where[0]), len(where), u, [i for i in range(n) if i != u]))
        exp_c = [true[s0:s0 + cnt][:, pres].contiguous() for (s0, cnt, u, pres) in runs]
        badp_c = torch.zeros((S, n - 1), dtype=torch.uint8, device=dev)

        def composed_mixed():
            for (s0, cnt, u, pres), e in zip(runs, exp_c):
                H._check(H.lib.hec_checksum_verify_device(
                    coder.handle, H.CHECKSUM_CRC32C, H._pp([ptrs[i] + s0 * stride for i in pres]),
                    H._sp([stride] * (n - 1)), n - 1, CELL, cnt, BPC, e.data_ptr(), badp_c.data_ptr() + s0 * (n - 1),
                    st))
            coder.scrub_device_mixed(ptrs, strides, masks, CELL, S, res_c.data_ptr(), ws_s.data_ptr(), ws_s.numel(),
                                     st)

        def fused_mixed():
            coder.scrub_crc_device_mixed(ptrs, strides, masks, CELL, S, true.data_ptr(), bad_f.data_ptr(),
                                         res_f.data_ptr(), ws_f.data_ptr(), ws_f.numel(), stream=st)

        bad_f.zero_()
        composed_mixed()
        fused_mixed()
        torch.cuda.synchronize()
        assert torch.equal(res_c, res_f) and not bool(res_f.any()), (name, "results")
        assert not bool(badp_c.any()) and not bool(bad_f.any()), (name, "flags")
        t_c, t_f = [], []
        for _ in range(ROUNDS):
            t_c.append(timed(stream, composed_mixed))
            t_f.append(timed(stream, fused_mixed))
        nbytes = (n - 1) * S * CELL
        print(f"{name}: {len(runs)} runs", flush=True)
        report(name, "verify + scrub_mixed", t_c, nbytes)
        report(name, "scrub_crc_mixed", t_f, nbytes)
        accept(name, t_c, t_f)
        coder.close()
        del cells, true, exp_c
        torch.cuda.empty_cache()


def accept(name, t_c, t_f):
    """DESIGN.md §3.4d's rule: the fused median no longer than the
    composition's median minus the composition's own round-to-round spread."""
    bound = statistics.median(t_c) - (max(t_c) - min(t_c))
    med = statistics.median(t_f)
    print(f"{name:28s} acceptance: fused median {med:.4f} ms vs composition median - spread {bound:.4f} ms: "
          f"{'PASS' if med <= bound else 'FAIL'} ({statistics.median(t_c) / med:.2f}x)", flush=True)


if __name__ == "__main__":
    main()
