"""Measurement probe (GPU box): the verified striped read into a file-order
buffer (hec_read_crc_rows_device[_mixed]: gf_read_rows) against the
composition out of calls that existed before it, on one MI355X, product
library, one process, the same buffers, CRC32C per 512-B chunk, a warm call,
rounds alternated, HIP events around REPS back-to-back repetitions.

Yardstick, a lost data unit in the batch: hec_reconstruct_crc_rows_device_mixed
with its outputs pointed at the file-order slots of a row-padded buffer (only
the lost data units wanted), behind one strided device copy per data unit over
all stripes (with a cycling loss that is 1/k more copy traffic than a reader
whose lost unit is the same in every stripe would have).  No
loss: hec_checksum_verify_device over the k data units plus the k copies.
Without d_expected the yardstick runs without it as well (no loss: the copies
alone).

Batch: RS(6,3) 1 MiB x 1024 and RS(10,4) 1 MiB x 256, with d_expected and
without, each in three shapes:
  (a) every stripe full, nothing lost;
  (b) every stripe full, one data unit lost per stripe, cycling;
  (c) every stripe short, r seeded uniform in [1, k * cell_len), one data unit
      lost per stripe, cycling.
Required for each: new median <= yardstick median + the yardstick's
round-to-round spread.  Also GB/s over the bytes the new call reads and writes.
  (d) RS(6,3): one group with only the last stripe short, uniform form, beside
      the same group without that stripe.  No bound: the extra launch.
The new call's file bytes (every byte of the row-padded buffer: the data
units' own bytes, the fill everywhere else) and flags are compared with the
true ones before anything is timed; the buffers and their truth are
probe_reconstruct_crc_rows.Batch's (zero-padded cells, the full-cell checksum
kernel and the CPU oracle's CRC of every short last chunk).
  python3 scripts/probe_read_crc_rows.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ec_oracle  # noqa: E402
import hdfs_native_ec as H  # noqa: E402
from probe_reconstruct_crc_rows import BPC, CELL, CONFIGS, ROUNDS, Batch, line, required, timed  # noqa: E402

FILL = 0xA5


class ReadBatch(Batch):
    """Batch with the file-order buffer of a read: [S, k, cell] (row-padded,
    stride k * cell), filled with 0xA5.  lost[s] is the data unit stripe s
    lacks, or None for no loss in the whole batch (the masks then have every
    unit, and the last parity unit's slot holds 0xEE: it is never read)."""

    def __init__(self, dev, gen, clib, k, m, S, cell, rs, lost):
        self.no_loss = lost is None
        super().__init__(dev, gen, clib, k, m, S, cell, BPC, rs, [k + m - 1] * S if lost is None else lost)
        n = k + m
        if self.no_loss:
            self.masks = [(1 << n) - 1] * S
        self.file = torch.full((S, k, cell), FILL, dtype=torch.uint8, device=dev)
        self.fptrs = [self.file.data_ptr() + u * cell for u in range(k)]
        self.fstrides = [k * cell] * k
        self.out_ptrs = self.fptrs + [None] * m
        self.out_strides = self.fstrides + [0] * m
        self.wants = [0 if self.no_loss else 1 << u for u in self.lost]
        pos = torch.arange(cell, device=dev, dtype=torch.int64)
        r = torch.tensor(rs, device=dev, dtype=torch.int64)
        self.exp_file = torch.full_like(self.file, FILL)
        moved = 0
        for u in range(k):
            ln = (r - u * cell).clamp(0, cell)
            self.exp_file[:, u] = torch.where(pos[None, :] < ln[:, None], self.exp_cells[:, u], self.exp_file[:, u])
            moved += 2 * int(ln.sum())
        self.moved = moved  # k reads + k writes of live bytes
        self.true_k = self.true[:, :k].contiguous()
        self.bad_k = torch.zeros((S, k), dtype=torch.uint8, device=dev)
        self.rws = torch.empty(self.coder.read_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

    def new(self, verify, st):
        self.coder.read_crc_rows_device_mixed(self.ptrs, self.strides, self.file.data_ptr(), self.masks, self.rs,
                                              self.cell, self.S, self.rws.data_ptr(), self.rws.numel(),
                                              expected_ptr=self.true.data_ptr() if verify else None,
                                              bad_ptr=self.bad.data_ptr(), bytes_per_checksum=BPC, stream=st)

    def yard(self, verify, st):
        k = self.k
        # one strided copy per data unit over all stripes; where the unit is
        # lost the copy carries its slot's 0xEE, which the repair then overwrites
        for u in range(k):
            self.file[:, u].copy_(self.cells[:, u])
        if self.no_loss:
            if verify:
                self.coder.checksum_verify_device(H.CHECKSUM_CRC32C, self.ptrs[:k], self.strides[:k], self.cell, self.S,
                                                  BPC, self.true_k.data_ptr(), self.bad_k.data_ptr(), st)
            return
        self.coder.reconstruct_crc_rows_device_mixed(
            self.ptrs, self.strides, self.out_ptrs, self.out_strides, self.masks, self.wants, self.rs, self.cell,
            self.S, self.sums.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
            expected_ptr=self.sums.data_ptr() if verify else None, bad_ptr=self.bad.data_ptr() if verify else None,
            bytes_per_checksum=BPC, stream=st)

    def check_file(self, what):
        torch.cuda.synchronize()
        assert not bool(self.bad.any()), (what, "flags")
        assert torch.equal(self.file, self.exp_file), (what, "file")
        self.file.fill_(FILL)


def compare(name, batch, stream, failed):
    st = stream.cuda_stream
    ts = {(label, verify): [] for label in ("yardstick", "new") for verify in (True, False)}
    for _ in range(ROUNDS):
        for verify in (True, False):
            ts[("yardstick", verify)].append(timed(stream, lambda: batch.yard(verify, st)))
            ts[("new", verify)].append(timed(stream, lambda: batch.new(verify, st)))
    for verify in (True, False):
        tag = "d_expected" if verify else "no d_expected"
        line(name, f"composition ({tag})", ts[("yardstick", verify)])
        line(name, f"read_crc_rows_device_mixed ({tag})", ts[("new", verify)], batch.moved)
        required(name, tag, ts[("yardstick", verify)], ts[("new", verify)], failed)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    rng = np.random.default_rng(17)
    clib = ec_oracle.load_c_oracle()
    failed = []
    for k, m, S in CONFIGS:
        full = k * CELL
        cycling = [s % k for s in range(S)]
        shapes = [("(a)", [full] * S, None), ("(b)", [full] * S, cycling),
                  ("(c)", [int(x) for x in rng.integers(1, full, size=S)], cycling)]
        for tag, rs, lost in shapes:
            name = f"{tag} RS({k},{m}) x {S}"
            b = ReadBatch(dev, gen, clib, k, m, S, CELL, rs, lost)
            for verify in (True, False):
                b.new(verify, st)
                b.check_file((name, "new", verify))
            print(f"{name:22s} bytes read and written by the new call: {b.moved} "
                  f"({b.moved / (2 * k * S * CELL):.3f} of the full cells')", flush=True)
            compare(name, b, stream, failed)
            del b
            torch.cuda.empty_cache()
        if (k, m) != (6, 3):
            continue
        # (d) only the last stripe short, uniform form
        r_last = 3 * CELL + 70001
        b = ReadBatch(dev, gen, clib, k, m, S, CELL, [full] * (S - 1) + [r_last], [1] * S)
        shards = [None if i == 1 else p for i, p in enumerate(b.ptrs)]

        def uniform(stripes, data_len):
            b.coder.read_crc_rows_device(shards, b.strides, b.file.data_ptr(), CELL, stripes, data_len=data_len,
                                         expected_ptr=b.true.data_ptr(), bad_ptr=b.bad.data_ptr(), stream=st)

        uniform(S, (S - 1) * full + r_last)
        b.check_file("(d) uniform form")
        tu, tf = [], []
        for _ in range(ROUNDS):
            tf.append(timed(stream, lambda: uniform(S - 1, 0)))
            tu.append(timed(stream, lambda: uniform(S, (S - 1) * full + r_last)))
        dname = f"(d) RS({k},{m}) x {S}"
        line(dname, f"read_crc_rows_device, {S - 1} full stripes", tf)
        line(dname, f"read_crc_rows_device, {S - 1} + 1 short", tu)
        print(f"{dname:22s} the extra launch: {(statistics.median(tu) - statistics.median(tf)) * 1e3:.1f} us", flush=True)
        del b
        torch.cuda.empty_cache()
    print("RESULT: " + ("every configuration within the bound" if not failed else f"missed the bound: {failed}"),
          flush=True)


if __name__ == "__main__":
    main()
