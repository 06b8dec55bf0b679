"""Measurement probe (GPU box): verified reconstruction of short stripes
(hec_reconstruct_crc_rows_device[_mixed]: gf_crc_rows<RowsRepair>) against
hec_reconstruct_crc_device[_mixed], on one MI355X, product library, one
process, the same buffers, CRC32C per 512-B chunk, a warm call, rounds
alternated, HIP events around REPS back-to-back repetitions.

Batch: RS(6,3) 1 MiB x 1024 and RS(10,4) 1 MiB x 256, one unit lost per stripe
(cycling over all units), with d_expected (== d_sums) and without.
  (a) every stripe full: the new mixed call against
      hec_reconstruct_crc_device_mixed.  Required: new median <= yardstick
      median + the yardstick's round-to-round spread.
  (b) every stripe short, r seeded uniform in [1, k * cell_len): the new mixed
      call against hec_reconstruct_crc_device_mixed over the same batch treated
      as full cells.  Required as (a).  Also GB/s and the share of the 8 TB/s
      peak over the bytes actually read and written, and the byte-wise route's
      rate on a 256-stripe slice (1024-B chunks are no fused shape).
  (c) one group of 1024 stripes with a short last stripe, uniform form, beside
      hec_reconstruct_crc_device on the 1023 full stripes.  No bound.
The new call's cells, sums and flags are compared with the true ones (built
from zero-padded cells, the full-cell checksum kernel and the CPU oracle's CRC
of every short last chunk) before anything is timed; the yardstick's outputs
are compared in (a), where they are the wanted ones.
  python3 scripts/probe_reconstruct_crc_rows.py
"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ec_oracle  # noqa: E402
import hdfs_native_ec as H  # noqa: E402

CELL = int(os.environ.get("PROBE_CELL", str(1 << 20)))
CONFIGS = [(6, 3, int(os.environ.get("PROBE_S63", "1024"))), (10, 4, int(os.environ.get("PROBE_S104", "256")))]
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "5"))
REPS = int(os.environ.get("PROBE_REPS", "8"))
BPC = 512
PEAK = 8e12  # HBM bytes/s
SCRIBBLE = 0x5A5A5A5A
GARBAGE = 0xEE


def timed(stream, fn):
    fn()  # warm: code objects, plan cache, staging
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(REPS):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS


def line(name, variant, ts, nbytes=None):
    med, lo, hi = statistics.median(ts), min(ts), max(ts)
    rate = "" if nbytes is None else (f"  {nbytes / (med * 1e-3) / 1e9:.0f} GB/s = {nbytes / (med * 1e-3) / PEAK:.3f} of peak "
                                      f"over the bytes read and written")
    print(f"{name:22s} {variant:44s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]{rate}", flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def required(name, tag, ty, tn, failed):
    bound = statistics.median(ty) + (max(ty) - min(ty))
    med = statistics.median(tn)
    ok = med <= bound
    if not ok:
        failed.append((name, tag))
    print(f"{name:22s} required ({tag}): new median {med:.4f} ms <= yardstick median + spread {bound:.4f} ms: "
          f"{'PASS' if ok else 'FAIL'} (yardstick / new = {statistics.median(ty) / med:.3f})", flush=True)


class Batch:
    """S stripes of RS(k,m), stripe s holding rs[s] logical bytes and lacking
    unit lost[s]: the buffers a caller has (0xEE from every unit's length on
    and in the lost slots, the survivors' live sums in the sums array) and
    the images a correct call leaves behind."""

    def __init__(self, dev, gen, clib, k, m, S, cell, bpc, rs, lost):
        n = k + m
        self.k, self.m, self.n, self.S, self.cell, self.bpc = k, m, n, S, cell, bpc
        self.coder = H.Coder(k, m, 0)
        st = torch.cuda.current_stream().cuda_stream
        pos = torch.arange(cell, device=dev, dtype=torch.int64)
        r = torch.tensor(rs, device=dev, dtype=torch.int64)
        lens = torch.empty((S, n), dtype=torch.int64, device=dev)
        for u in range(n):
            lens[:, u] = (r - u * cell).clamp(0, cell) if u < k else r.clamp(max=cell)
        cells = torch.empty((S, n, cell), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=gen)
        for u in range(k):  # zero-padded data, then its parity
            cells[:, u].masked_fill_(pos[None, :] >= lens[:, u, None], 0)
        self.ptrs, self.strides = H.stripe_layout_ptrs(cells, n)
        self.coder.encode_device(self.ptrs[:k], self.strides[:k], self.ptrs[k:], self.strides[k:], cell, S, st)
        nck = -(-cell // bpc)
        full = torch.empty((S, n, nck), dtype=torch.int32, device=dev)
        H._check(H.lib.hec_checksum_device(self.coder.handle, H.CHECKSUM_CRC32C, H._pp(self.ptrs), H._sp(self.strides),
                                           n, cell, S, bpc, full.data_ptr(), st))
        torch.cuda.synchronize()
        # the true sums over every unit's own bytes: the full chunks' from the
        # checksum kernel, every short last chunk's from the CPU oracle
        chunk = torch.arange(nck, device=dev, dtype=torch.int64)
        live = chunk[None, None, :] * bpc < lens[:, :, None]
        self.true = torch.where(live, full, torch.full_like(full, SCRIBBLE))
        lens_h = lens.cpu().numpy()
        short = [(s, u) for s in range(S) for u in range(n) if lens_h[s, u] % bpc]
        if short:
            tails = torch.zeros((len(short), bpc), dtype=torch.uint8, device=dev)
            for i, (s, u) in enumerate(short):
                ln = int(lens_h[s, u])
                tails[i, :ln % bpc] = cells[s, u, ln - ln % bpc:ln]
            tails_h = tails.cpu().numpy()
            words = np.empty(len(short), dtype=np.int32)
            for i, (s, u) in enumerate(short):
                row = np.ascontiguousarray(tails_h[i, :int(lens_h[s, u]) % bpc])
                crc = clib.orc_crc32c(row.ctypes.data_as(ctypes.c_void_p), row.size)
                words[i] = np.frombuffer(int(crc).to_bytes(4, "big"), dtype=np.int32)[0]
            idx = torch.tensor(short, device=dev, dtype=torch.int64)
            self.true[idx[:, 0], idx[:, 1], torch.tensor([int(lens_h[s, u]) // bpc for s, u in short], device=dev)] = \
                torch.from_numpy(words).to(dev)
        # the expected cells: the unit's bytes, zeros up to n0 in the rebuilt slot, 0xEE elsewhere
        n0 = r.clamp(max=cell)
        self.exp_cells = cells.clone()
        sidx = torch.arange(S, device=dev)
        lost_t = torch.tensor(lost, device=dev, dtype=torch.int64)
        for u in range(n):
            cells[:, u].masked_fill_(pos[None, :] >= lens[:, u, None], GARBAGE)
            keep = torch.where(lost_t == u, n0, lens[:, u])
            self.exp_cells[:, u].masked_fill_(pos[None, :] >= keep[:, None], GARBAGE)
        cells[sidx, lost_t] = GARBAGE
        self.cells = cells
        self.lost, self.rs = lost, rs
        self.masks = [((1 << n) - 1) & ~(1 << u) for u in lost]
        self.sums = self.true.clone()
        self.sums[sidx, lost_t] = SCRIBBLE
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(self.coder.reconstruct_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        # bytes a one-pass call moves: the k survivors' and the target's (up to n0)
        moved = 0
        for s in range(S):
            surv = [u for u in range(n) if u != lost[s]][:k]
            moved += int(sum(lens_h[s, u] for u in surv)) + min(cell, rs[s])
        self.moved = moved

    def new(self, verify, st, stripe_bytes="rs"):
        self.coder.reconstruct_crc_rows_device_mixed(
            self.ptrs, self.strides, self.ptrs, self.strides, self.masks, None,
            self.rs if stripe_bytes == "rs" else stripe_bytes, self.cell, self.S, self.sums.data_ptr(),
            self.ws.data_ptr(), self.ws.numel(), expected_ptr=self.sums.data_ptr() if verify else None,
            bad_ptr=self.bad.data_ptr() if verify else None, bytes_per_checksum=self.bpc, stream=st)

    def yard(self, verify, st):
        self.coder.reconstruct_crc_device_mixed(
            self.ptrs, self.strides, self.ptrs, self.strides, self.masks, None, self.cell, self.S,
            self.sums.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            expected_ptr=self.sums.data_ptr() if verify else None, bad_ptr=self.bad.data_ptr() if verify else None,
            bytes_per_checksum=self.bpc, stream=st)

    def reset(self):
        sidx = torch.arange(self.S, device=self.cells.device)
        lost_t = torch.tensor(self.lost, device=self.cells.device, dtype=torch.int64)
        self.cells[sidx, lost_t] = GARBAGE
        self.sums.copy_(self.true)
        self.sums[sidx, lost_t] = SCRIBBLE
        self.bad.zero_()

    def check(self, what):
        torch.cuda.synchronize()
        assert not bool(self.bad.any()), (what, "flags")
        assert torch.equal(self.sums, self.true), (what, "sums")
        assert torch.equal(self.cells, self.exp_cells), (what, "cells")


def compare(name, batch, stream, failed, info_bytes):
    st = stream.cuda_stream
    ts = {(label, verify): [] for label in ("yardstick", "new") for verify in (True, False)}
    for _ in range(ROUNDS):
        for verify in (True, False):
            ts[("yardstick", verify)].append(timed(stream, lambda: batch.yard(verify, st)))
            ts[("new", verify)].append(timed(stream, lambda: batch.new(verify, st)))
    for verify in (True, False):
        tag = "d_expected" if verify else "no d_expected"
        line(name, f"reconstruct_crc_device_mixed ({tag})", ts[("yardstick", verify)])
        line(name, f"reconstruct_crc_rows_device_mixed ({tag})", ts[("new", verify)], info_bytes)
        required(name, tag, ts[("yardstick", verify)], ts[("new", verify)], failed)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    rng = np.random.default_rng(11)
    clib = ec_oracle.load_c_oracle()
    failed = []
    for k, m, S in CONFIGS:
        n, full = k + m, k * CELL
        lost = [s % n for s in range(S)]
        # (a) every stripe full
        name = f"(a) RS({k},{m}) x {S}"
        b = Batch(dev, gen, clib, k, m, S, CELL, BPC, [full] * S, lost)
        for label, fn in (("yardstick", lambda v: b.yard(v, st)), ("new", lambda v: b.new(v, st)),
                          ("new, stripe_bytes NULL", lambda v: b.new(v, st, None))):
            for verify in (True, False):
                b.reset()
                fn(verify)
                b.check((name, label, verify))
        compare(name, b, stream, failed, b.moved)
        # (c) one group with a short last stripe, uniform form (RS(6,3) only)
        if (k, m) == (6, 3):
            del b
            torch.cuda.empty_cache()
            r_last = 3 * CELL + 70001
            b = Batch(dev, gen, clib, k, m, S, CELL, BPC, [full] * (S - 1) + [r_last], [1] * S)
            shards = [None if i == 1 else p for i, p in enumerate(b.ptrs)]
            data_len = (S - 1) * full + r_last

            def rows_uniform():
                b.coder.reconstruct_crc_rows_device(shards, b.strides, b.ptrs, b.strides, CELL, S, b.sums.data_ptr(),
                                                    data_len=data_len, expected_ptr=b.sums.data_ptr(),
                                                    bad_ptr=b.bad.data_ptr(), stream=st)

            def full_uniform():
                b.coder.reconstruct_crc_device(shards, b.strides, b.ptrs, b.strides, CELL, S - 1, b.sums.data_ptr(),
                                               expected_ptr=b.sums.data_ptr(), bad_ptr=b.bad.data_ptr(), stream=st)

            b.reset()
            rows_uniform()
            b.check("(c) uniform form")
            tu, tf = [], []
            for _ in range(ROUNDS):
                tf.append(timed(stream, full_uniform))
                tu.append(timed(stream, rows_uniform))
            cname = f"(c) RS({k},{m}) x {S}"
            line(cname, f"reconstruct_crc_device, {S - 1} full stripes", tf)
            line(cname, f"reconstruct_crc_rows_device, {S - 1} + 1 short", tu)
            print(f"{cname:22s} the extra launch: {(statistics.median(tu) - statistics.median(tf)) * 1e3:.1f} us",
                  flush=True)
        del b
        torch.cuda.empty_cache()
        # (b) every stripe short
        name = f"(b) RS({k},{m}) x {S}"
        rs = [int(x) for x in rng.integers(1, full, size=S)]
        b = Batch(dev, gen, clib, k, m, S, CELL, BPC, rs, lost)
        for verify in (True, False):
            b.reset()
            b.new(verify, st)
            b.check((name, "new", verify))
        print(f"{name:22s} bytes read and written by a one-pass call: {b.moved} "
              f"({b.moved / ((k + 1) * S * CELL):.3f} of the full cells')", flush=True)
        compare(name, b, stream, failed, b.moved)
        del b
        torch.cuda.empty_cache()
    # the byte-wise route, once, for information: 1024-B chunks are no fused shape
    k, m, S, bpc = 6, 3, 256, 1024
    rs = [int(x) for x in rng.integers(1, k * CELL, size=S)]
    b = Batch(dev, gen, clib, k, m, S, CELL, bpc, rs, [s % (k + m) for s in range(S)])
    b.reset()
    b.new(True, st)
    b.check("byte-wise route")
    tg = [timed(stream, lambda: b.new(True, st)) for _ in range(ROUNDS)]
    line(f"RS({k},{m}) x {S} bpc {bpc}", "reconstruct_crc_rows_device_mixed (byte-wise)", tg, b.moved)
    print("RESULT: " + ("every configuration within the bound" if not failed else f"missed the bound: {failed}"),
          flush=True)


if __name__ == "__main__":
    main()
