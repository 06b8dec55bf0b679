"""Measurement probe (GPU box): encode with chunk sums of short stripes
(hec_encode_crc_rows_device[_mixed]: gf_crc_rows<RowsEncode>) against what a caller
pays without it, hec_encode_crc_device over the same stripes zero-padded and
treated as full cells (a yardstick for time only: its sums of cut units are not
the wanted ones).  One MI355X, product library, one process, the same buffers,
CRC32C per 512-B chunk, a warm call, rounds alternated, HIP events around REPS
back-to-back repetitions, medians.

Batch: RS(6,3) 1 MiB x 1024 and RS(10,4) 1 MiB x 256.
  (a)  every stripe full, uniform form (data_len == 0): the same launches as
       hec_encode_crc_device, so it must tie.
  (a') the same full stripes forced through gf_crc_rows<RowsEncode>: the mixed form
       with one short stripe appended, against hec_encode_crc_device over all
       of them.  What a full stripe costs in the rows kernel.
  (b)  every stripe short, r seeded uniform in [1, k * cell_len), mixed form.
       Also GB/s and the share of the 8 TB/s peak over the bytes moved.
       PROBE_R_ALIGN=512 rounds every r down to a multiple of 512, so that no
       unit has a short last chunk.
  (c)  one group with a short last stripe, uniform form, beside
       hec_encode_crc_device on the stripes - 1 full stripes: the cost of the
       extra launch.  No bound.
Required for (a), (a'), (b): new median <= yardstick median + the yardstick's
round-to-round spread.
Before anything is timed both sides are checked: the parity against
hec_encode_device's over the zero-padded cells (and the CPU oracle's on sampled
stripes), below n0 for the new call with the 0xA5 fill intact behind it; the
new call's sums against hec_checksum_device's over each unit's whole chunks and
the CPU oracle's over every short last chunk, the scribble intact in every dead
slot; the yardstick's sums against hec_checksum_device's of the padded cells.
  python3 scripts/probe_encode_crc_rows.py
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
OUTFILL = 0xA5


def timed(stream, fn):
    fn()  # warm: code objects, staging
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
                                      f"over the bytes moved")
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
    """S stripes of RS(k,m), stripe s holding rs[s] logical bytes, the data
    slots zero-padded behind every unit's length (what the yardstick needs and
    what the new call ignores).  ref_par: hec_encode_device's parity of them;
    sums_pad: hec_checksum_device's sums of the padded cells as full cells;
    sums_own: every unit's sums over its own bytes, a scribble behind its live
    chunks."""

    def __init__(self, dev, gen, clib, k, m, S, cell, rs):
        n = k + m
        self.k, self.m, self.n, self.S, self.cell, self.rs = k, m, n, S, cell, rs
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
        self.dp, self.ds, self.pp, self.ps = self.ptrs[:k], self.strides[:k], self.ptrs[k:], self.strides[k:]
        self.coder.encode_device(self.dp, self.ds, self.pp, self.ps, cell, S, st)
        nck = -(-cell // BPC)
        full = torch.empty((S, n, nck), dtype=torch.int32, device=dev)
        H._check(H.lib.hec_checksum_device(self.coder.handle, H.CHECKSUM_CRC32C, H._pp(self.ptrs), H._sp(self.strides),
                                           n, cell, S, BPC, full.data_ptr(), st))
        torch.cuda.synchronize()
        self.ref_par = cells[:, k:].clone()
        # sampled stripes against the CPU oracle's parity
        for s in sorted({0, S // 2, S - 1}):
            host = cells[s].cpu().numpy()
            want = ec_oracle.c_encode(clib, k, m, [np.ascontiguousarray(host[i]) for i in range(k)])
            for j in range(m):
                assert np.array_equal(host[k + j], want[j]), ("reference parity", s, j)
        self.sums_pad = full
        chunk = torch.arange(nck, device=dev, dtype=torch.int64)
        self.live = chunk[None, None, :] * BPC < lens[:, :, None]
        self.sums_own = torch.where(self.live, full, torch.full_like(full, SCRIBBLE))
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
        self.cells, self.lens, self.lens_h = cells, lens, lens_h
        self.n0 = r.clamp(max=cell)
        self.pos = pos
        self.sums = torch.empty((S, n, nck), dtype=torch.int32, device=dev)
        self.ws = torch.empty(max(8, self.coder.encode_crc_rows_mixed_workspace_size(S)), dtype=torch.uint8, device=dev)

    def moved(self, stripes=None):
        """Bytes a one-pass call reads and writes: every unit's own bytes."""
        return int(self.lens_h[:stripes].sum())

    def yard(self, st, stripes=None):
        self.coder.encode_crc_device(self.dp, self.ds, self.pp, self.ps, self.cell, self.S if stripes is None else stripes,
                                     BPC, self.sums.data_ptr(), st)

    def uniform(self, st, stripes, data_len):
        self.coder.encode_crc_rows_device(self.dp, self.ds, self.pp, self.ps, self.cell, stripes, self.sums.data_ptr(),
                                          data_len=data_len, stream=st)

    def mixed(self, st, stripe_bytes):
        self.coder.encode_crc_rows_device_mixed(self.dp, self.ds, self.pp, self.ps, stripe_bytes, self.cell, self.S,
                                                self.sums.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream=st)

    def check(self, what, fn, own, stripes=None):
        """fn on 0xA5-filled parity slots and scribbled sums.  own: the outputs
        of the new calls (parity below n0 and nothing behind, every unit's own
        sums and nothing in a dead slot); else the full cells' parity and sums."""
        S = self.S if stripes is None else stripes
        par = self.cells[:, self.k:]
        par.fill_(OUTFILL)
        self.sums.fill_(SCRIBBLE)
        fn()
        torch.cuda.synchronize()
        if own:
            below = self.pos[None, None, :] < self.n0[:, None, None]
            want = torch.where(below, self.ref_par, torch.full_like(self.ref_par, OUTFILL))
            want_sums = self.sums_own
        else:
            want, want_sums = self.ref_par, self.sums_pad
        assert torch.equal(par[:S], want[:S]), (what, "parity")
        assert bool((par[S:] == OUTFILL).all()), (what, "parity behind the call's stripes")
        assert torch.equal(self.sums[:S], want_sums[:S]), (what, "sums")
        assert bool((self.sums[S:] == SCRIBBLE).all()), (what, "sums behind the call's stripes")
        par.copy_(self.ref_par)


def compare(name, stream, yard, new, failed, nbytes=None, bound=True):
    ty, tn = [], []
    for _ in range(ROUNDS):
        ty.append(timed(stream, yard))
        tn.append(timed(stream, new))
    line(name, "yardstick", ty)
    line(name, "new", tn, nbytes)
    if bound:
        required(name, ty, tn, failed)
    else:
        print(f"{name:34s} the extra launch: {(statistics.median(tn) - statistics.median(ty)) * 1e3:.1f} us", flush=True)


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
        # (a), (a'), (c): S full stripes and one short stripe behind them
        r_last = (k // 2) * CELL + 70001
        b = Batch(dev, gen, clib, k, m, S + 1, CELL, [full] * S + [r_last])
        name = f"(a) RS({k},{m}) x {S} uniform form"
        b.check((name, "yardstick"), lambda: b.yard(st, S), False, S)
        b.check((name, "new"), lambda: b.uniform(st, S, 0), True, S)
        compare(name, stream, lambda: b.yard(st, S), lambda: b.uniform(st, S, 0), failed, b.moved(S))
        name = f"(a') RS({k},{m}) x {S} + 1 rows kernel"
        lens = [0] * S + [r_last]
        b.check((name, "yardstick"), lambda: b.yard(st), False)
        b.check((name, "new"), lambda: b.mixed(st, lens), True)
        compare(name, stream, lambda: b.yard(st), lambda: b.mixed(st, lens), failed, b.moved())
        name = f"(c) RS({k},{m}) x {S} + 1 short, uniform"
        data_len = S * full + r_last
        b.check((name, "new"), lambda: b.uniform(st, S + 1, data_len), True)
        compare(name, stream, lambda: b.yard(st, S), lambda: b.uniform(st, S + 1, data_len), failed, bound=False)
        del b
        torch.cuda.empty_cache()
        # (b) every stripe short
        rs = [max(R_ALIGN, int(x) // R_ALIGN * R_ALIGN) for x in rng.integers(1, full, size=S)]
        b = Batch(dev, gen, clib, k, m, S, CELL, rs)
        name = f"(b) RS({k},{m}) x {S} every stripe short"
        b.check((name, "yardstick"), lambda: b.yard(st), False)
        b.check((name, "new"), lambda: b.mixed(st, rs), True)
        moved = b.moved()
        print(f"{name:34s} bytes moved by a one-pass call: {moved} ({moved / (S * (k + m) * CELL):.3f} of the full cells')",
              flush=True)
        compare(name, stream, lambda: b.yard(st), lambda: b.mixed(st, rs), failed, moved)
        del b
        torch.cuda.empty_cache()
    print("RESULT: " + ("every row within its bound" if not failed else f"missed the bound: {failed}"), flush=True)


if __name__ == "__main__":
    main()
