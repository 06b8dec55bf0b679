"""Measurement probe (GPU box): checksum-only reconstruction
(hec_reconstruct_sums_device: gf_reconstruct_crc without its output stores)
against what a caller had to do before it for the same sums, on one MI355X,
product library, one process, the same buffers, a warm call, rounds
alternated, HIP events around REPS back-to-back repetitions.

The yardstick: hec_reconstruct_crc_device with d_out pointing at a scratch
buffer of stripes x t x cell_len bytes that nobody reads.  Configurations, CRC32C
per 512-B chunk: RS(6,3) 1 MiB x 1024 with one data unit, one parity unit and
three units lost, RS(10,4) 1 MiB x 256 with one unit lost; each with
d_expected (== d_sums) and without.  Required: the new call's median is no
longer than the yardstick's median plus the yardstick's own round-to-round
spread (max - min of its round medians).  Both calls are checked against the
true sums before anything is timed.  Last, for information, the rate of the
generic kernel (gf_reconstruct_sums_bytes) on a shape the fused one does not
take.
  python3 scripts/probe_reconstruct_sums.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))

import torch  # noqa: E402

import hdfs_native_ec as H  # noqa: E402

CELL = int(os.environ.get("PROBE_CELL", str(1 << 20)))
CONFIGS = [(6, 3, 1024, (1,)), (6, 3, 1024, (7,)), (6, 3, 1024, (1, 4, 7)), (10, 4, 256, (3,))]
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "5"))
REPS = int(os.environ.get("PROBE_REPS", "8"))
BPC = 512
PEAK = 8e12  # HBM bytes/s
SCRIBBLE = 0x5A5A5A5A


def timed(stream, fn):
    fn()  # warm: code objects, plan cache
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def line(name, variant, ts, nbytes):
    med, lo, hi = statistics.median(ts), min(ts), max(ts)
    print(f"{name:28s} {variant:36s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
          f"{nbytes / (med * 1e-3) / PEAK:.3f} of peak over k reads", flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def group(dev, gen, k, m, S, cell, bpc):
    """Encoded cells [S, n, cell] and the true sums of every cell [S, n, nck]."""
    n = k + m
    coder = H.Coder(k, m, 0)
    st = torch.cuda.current_stream().cuda_stream
    cells = torch.empty((S, n, cell), dtype=torch.uint8, device=dev)
    cells.random_(0, 256, generator=gen)
    ptrs, strides = H.stripe_layout_ptrs(cells, n)
    coder.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], cell, S, st)
    true = torch.empty((S, n, -(-cell // bpc)), dtype=torch.int32, device=dev)
    H._check(H.lib.hec_checksum_device(coder.handle, H.CHECKSUM_CRC32C, H._pp(ptrs), H._sp(strides), n, cell, S, bpc,
                                       true.data_ptr(), st))
    torch.cuda.synchronize()
    return coder, cells, ptrs, strides, true


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    built = {}
    failed = []
    for k, m, S, lost in CONFIGS:
        n, t = k + m, len(lost)
        name = f"RS({k},{m}) x {S} lost {','.join(map(str, lost))}"
        if (k, m, S) not in built:
            built.clear()
            torch.cuda.empty_cache()
            built[(k, m, S)] = group(dev, gen, k, m, S, CELL, BPC)
        coder, cells, ptrs, strides, true = built[(k, m, S)]
        shards = [None if i in lost else ptrs[i] for i in range(n)]
        # the yardstick's scratch: one cell per target and stripe, never read
        scratch = torch.empty((S, t, CELL), dtype=torch.uint8, device=dev)
        optrs, ostrides = [0] * n, [0] * n
        for j, u in enumerate(lost):
            optrs[u], ostrides[u] = scratch.data_ptr() + j * CELL, t * CELL
        sums = true.clone()
        bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)

        def yard(verify):
            coder.reconstruct_crc_device(shards, strides, optrs, ostrides, CELL, S, sums.data_ptr(),
                                         expected_ptr=sums.data_ptr() if verify else None,
                                         bad_ptr=bad.data_ptr() if verify else None, bytes_per_checksum=BPC, stream=st)

        def new(verify):
            coder.reconstruct_sums_device(shards, strides, CELL, S, sums.data_ptr(),
                                          expected_ptr=sums.data_ptr() if verify else None,
                                          bad_ptr=bad.data_ptr() if verify else None, bytes_per_checksum=BPC, stream=st)

        for label, fn in (("yardstick", yard), ("new", new)):
            for verify in (True, False):
                sums[:, list(lost)] = SCRIBBLE
                fn(verify)
                torch.cuda.synchronize()
                assert torch.equal(sums, true), (name, label, verify, "sums")
                assert not bool(bad.any()), (name, label, verify, "flags")
        ts = {(label, verify): [] for label in ("yardstick", "new") for verify in (True, False)}
        for _ in range(ROUNDS):
            for verify in (True, False):
                ts[("yardstick", verify)].append(timed(stream, lambda: yard(verify)))
                ts[("new", verify)].append(timed(stream, lambda: new(verify)))
        nbytes = k * S * CELL
        print(f"{name}: yardstick scratch {scratch.numel()} bytes ({scratch.numel() / 2**30:.2f} GiB)", flush=True)
        for verify in (True, False):
            tag = "d_expected" if verify else "no d_expected"
            ty, tn = ts[("yardstick", verify)], ts[("new", verify)]
            line(name, f"reconstruct_crc -> scratch ({tag})", ty, nbytes)
            line(name, f"reconstruct_sums ({tag})", tn, nbytes)
            bound = statistics.median(ty) + (max(ty) - min(ty))
            med = statistics.median(tn)
            ok = med <= bound
            if not ok:
                failed.append((name, tag))
            print(f"{name:28s} required ({tag}): new median {med:.4f} ms <= yardstick median + spread {bound:.4f} ms: "
                  f"{'PASS' if ok else 'FAIL'} (yardstick / new = {statistics.median(ty) / med:.3f})", flush=True)
        del scratch, sums
    built.clear()
    torch.cuda.empty_cache()
    # the generic kernel, once, for information: 1024-B chunks are no fused shape
    k, m, S, lost, bpc = 6, 3, 256, (1,), 1024
    coder, cells, ptrs, strides, true = group(dev, gen, k, m, S, CELL, bpc)
    shards = [None if i in lost else ptrs[i] for i in range(k + m)]
    sums = true.clone()
    sums[:, list(lost)] = SCRIBBLE

    def generic():
        coder.reconstruct_sums_device(shards, strides, CELL, S, sums.data_ptr(), bytes_per_checksum=bpc, stream=st)

    generic()
    torch.cuda.synchronize()
    assert torch.equal(sums, true), "generic sums"
    tg = [timed(stream, generic) for _ in range(ROUNDS)]
    line(f"RS({k},{m}) x {S} lost 1, bpc {bpc}", "reconstruct_sums (generic kernel)", tg, k * S * CELL)
    print(f"  generic kernel: {k * S * CELL / (statistics.median(tg) * 1e-3) / 1e9:.1f} GB/s of survivor bytes",
          flush=True)
    print("RESULT: " + ("every configuration within the bound" if not failed else f"missed the bound: {failed}"),
          flush=True)


if __name__ == "__main__":
    main()
