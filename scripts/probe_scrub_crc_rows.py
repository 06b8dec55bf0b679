"""Measurement probe (GPU box): verified scrub of short stripes
(hec_scrub_crc_rows_device[_mixed]: gf_scrub_crc_rows) against
hec_scrub_crc_device[_mixed], on one MI355X, product library, one process, the
same buffers, CRC32C per 512-B chunk, a warm call, rounds alternated, HIP
events around REPS back-to-back repetitions.

Batch: RS(6,3) 1 MiB x 1024 and RS(10,4) 1 MiB x 256; every unit present, and
a node-failure batch with one unit lost per stripe (cycling over all units).
  (a) every stripe full: the new mixed call against hec_scrub_crc_device_mixed
      (and the new uniform call against hec_scrub_crc_device, every unit
      present).  Required: new median <= yardstick median + the yardstick's
      round-to-round spread.
  (b) every stripe short, r seeded uniform in [1, k * cell_len): the new mixed
      call against hec_scrub_crc_device_mixed over the same zero-padded cells
      treated as full cells, with sums of the padded cells for the yardstick
      only.  Required as (a).  Also GB/s and the share of the 8 TB/s peak over
      the bytes actually read.
      PROBE_R_ALIGN=512 rounds every r down to a multiple of 512, so that no
      unit has a short last chunk.
  (c) one group with a short last stripe, uniform form, beside
      hec_scrub_crc_device on the stripes - 1 full stripes.  No bound.
The batches are clean: the results (pre-filled with -1) must come back (0, 0)
and the flags stay zero on both sides before anything is timed.
  python3 scripts/probe_scrub_crc_rows.py
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
R_ALIGN = int(os.environ.get("PROBE_R_ALIGN", "1"))  # (b): r rounded down to a multiple of it (512: no short last chunk)
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
                                      f"over the bytes read")
    print(f"{name:34s} {variant:40s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]{rate}", flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def required(name, ty, tn, failed):
    bound = statistics.median(ty) + (max(ty) - min(ty))
    med = statistics.median(tn)
    ok = med <= bound
    if not ok:
        failed.append(name)
    print(f"{name:34s} required: new median {med:.4f} ms <= yardstick median + spread {bound:.4f} ms: "
          f"{'PASS' if ok else 'MISSED'} (yardstick / new = {statistics.median(ty) / med:.3f})", flush=True)


class Batch:
    """S clean stripes of RS(k,m), stripe s holding rs[s] logical bytes, the
    slots zero-padded behind every unit's length (what the yardstick needs and
    what the new call ignores).  sums_own: every unit's sums over its own
    bytes, a scribble behind its live chunks; sums_pad: the sums of the padded
    cells as full cells."""

    def __init__(self, dev, gen, clib, k, m, S, cell, rs):
        n = k + m
        self.k, self.m, self.n, self.S, self.cell = k, m, n, S, cell
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
        nck = -(-cell // BPC)
        full = torch.empty((S, n, nck), dtype=torch.int32, device=dev)
        H._check(H.lib.hec_checksum_device(self.coder.handle, H.CHECKSUM_CRC32C, H._pp(self.ptrs), H._sp(self.strides),
                                           n, cell, S, BPC, full.data_ptr(), st))
        torch.cuda.synchronize()
        self.sums_pad = full
        chunk = torch.arange(nck, device=dev, dtype=torch.int64)
        live = chunk[None, None, :] * BPC < lens[:, :, None]
        self.sums_own = torch.where(live, full, torch.full_like(full, SCRIBBLE))
        lens_h = lens.cpu().numpy()
        short = [(s, u) for s in range(S) for u in range(n) if lens_h[s, u] % BPC]
        if short:  # every short last chunk's sum from the CPU oracle
            tails = torch.zeros((len(short), BPC), dtype=torch.uint8, device=dev)
            for i, (s, u) in enumerate(short):
                ln = int(lens_h[s, u])
                tails[i, :ln % BPC] = cells[s, u, ln - ln % BPC:ln]
            tails_h = tails.cpu().numpy()
            words = np.empty(len(short), dtype=np.int32)
            for i, (s, u) in enumerate(short):
                row = np.ascontiguousarray(tails_h[i, :int(lens_h[s, u]) % BPC])
                crc = clib.orc_crc32c(row.ctypes.data_as(ctypes.c_void_p), row.size)
                words[i] = np.frombuffer(int(crc).to_bytes(4, "big"), dtype=np.int32)[0]
            idx = torch.tensor(short, device=dev, dtype=torch.int64)
            self.sums_own[idx[:, 0], idx[:, 1],
                          torch.tensor([int(lens_h[s, u]) // BPC for s, u in short], device=dev)] = \
                torch.from_numpy(words).to(dev)
        self.cells, self.rs, self.lens_h = cells, rs, lens_h
        self.res = torch.empty((S, 2), dtype=torch.int64, device=dev)
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(self.coder.scrub_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

    def moved(self, masks):
        return int(sum(self.lens_h[s, u] for s in range(self.S) for u in range(self.n) if (masks[s] >> u) & 1))

    def new(self, masks, st, stripe_bytes="rs"):
        self.coder.scrub_crc_rows_device_mixed(self.ptrs, self.strides, masks,
                                               self.rs if stripe_bytes == "rs" else stripe_bytes, self.cell, self.S,
                                               self.sums_own.data_ptr(), self.bad.data_ptr(), self.res.data_ptr(),
                                               self.ws.data_ptr(), self.ws.numel(), stream=st)

    def yard(self, masks, st):
        self.coder.scrub_crc_device_mixed(self.ptrs, self.strides, masks, self.cell, self.S, self.sums_pad.data_ptr(),
                                          self.bad.data_ptr(), self.res.data_ptr(), self.ws.data_ptr(),
                                          self.ws.numel(), stream=st)

    def clean(self, what, fn):
        self.res.fill_(-1)
        self.bad.zero_()
        fn()
        torch.cuda.synchronize()
        assert not bool(self.res.any()), (what, "results", self.res.nonzero()[:8].tolist())
        assert not bool(self.bad.any()), (what, "flags", self.bad.nonzero()[:8].tolist())


def compare(name, stream, yard, new, failed, nbytes=None):
    ty, tn = [], []
    for _ in range(ROUNDS):
        ty.append(timed(stream, yard))
        tn.append(timed(stream, new))
    line(name, "yardstick", ty)
    line(name, "new", tn, nbytes)
    required(name, ty, tn, failed)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(13)
    rng = np.random.default_rng(13)
    clib = ec_oracle.load_c_oracle()
    failed = []
    for k, m, S in CONFIGS:
        n, full = k + m, k * CELL
        every = [(1 << n) - 1] * S
        node = [((1 << n) - 1) & ~(1 << (s % n)) for s in range(S)]
        # (a) every stripe full
        b = Batch(dev, gen, clib, k, m, S, CELL, [full] * S)
        for mname, masks in (("all present", every), ("node failure", node)):
            name = f"(a) RS({k},{m}) x {S} {mname}"
            b.clean((name, "yardstick"), lambda: b.yard(masks, st))
            b.clean((name, "new"), lambda: b.new(masks, st))
            b.clean((name, "new, stripe_bytes NULL"), lambda: b.new(masks, st, None))
            compare(name, stream, lambda: b.yard(masks, st), lambda: b.new(masks, st), failed, b.moved(masks))

        def uni(stripes, data_len=None):
            if data_len is None:
                b.coder.scrub_crc_device(b.ptrs, b.strides, CELL, stripes, b.sums_own.data_ptr(), b.bad.data_ptr(),
                                         b.res.data_ptr(), stream=st)
            else:
                b.coder.scrub_crc_rows_device(b.ptrs, b.strides, CELL, stripes, b.sums_own.data_ptr(),
                                              b.bad.data_ptr(), b.res.data_ptr(), data_len=data_len, stream=st)

        name = f"(a) RS({k},{m}) x {S} uniform form"
        b.clean((name, "yardstick"), lambda: uni(S))
        b.clean((name, "new"), lambda: uni(S, 0))
        compare(name, stream, lambda: uni(S), lambda: uni(S, 0), failed, b.moved(every))
        del b
        torch.cuda.empty_cache()
        # (c) one group with a short last stripe, uniform form
        r_last = (k // 2) * CELL + 70001
        b = Batch(dev, gen, clib, k, m, S, CELL, [full] * (S - 1) + [r_last])
        data_len = (S - 1) * full + r_last
        cname = f"(c) RS({k},{m}) x {S}"
        b.clean((cname, "new"), lambda: uni(S, data_len))
        tf, tu = [], []
        for _ in range(ROUNDS):
            tf.append(timed(stream, lambda: uni(S - 1)))
            tu.append(timed(stream, lambda: uni(S, data_len)))
        line(cname, f"scrub_crc_device, {S - 1} full stripes", tf)
        line(cname, f"scrub_crc_rows_device, {S - 1} + 1 short", tu)
        print(f"{cname:34s} the extra launch: {(statistics.median(tu) - statistics.median(tf)) * 1e3:.1f} us", flush=True)
        del b
        torch.cuda.empty_cache()
        # (b) every stripe short
        rs = [max(R_ALIGN, int(x) // R_ALIGN * R_ALIGN) for x in rng.integers(1, full, size=S)]
        b = Batch(dev, gen, clib, k, m, S, CELL, rs)
        for mname, masks in (("all present", every), ("node failure", node)):
            name = f"(b) RS({k},{m}) x {S} {mname}"
            b.clean((name, "yardstick"), lambda: b.yard(masks, st))
            b.clean((name, "new"), lambda: b.new(masks, st))
            moved = b.moved(masks)
            cells_read = sum(bin(x).count("1") for x in masks) * CELL
            print(f"{name:34s} bytes read by a one-pass call: {moved} ({moved / cells_read:.3f} of the full cells')",
                  flush=True)
            compare(name, stream, lambda: b.yard(masks, st), lambda: b.new(masks, st), failed, moved)
        del b
        torch.cuda.empty_cache()
    print("RESULT: " + ("every row within its bound" if not failed else f"missed the bound: {failed}"), flush=True)


if __name__ == "__main__":
    main()
