"""Measurement probe (GPU box): the mixed-pattern reconstruction
(hec_reconstruct_device_mixed, kernel gf_reconstruct_mixed) on one MI355X,
product library, one process, the same buffers, rounds alternated, HIP events
around REPS back-to-back calls (workspace upload included, as a caller pays
it).  Per config, RS(6,3) 1 MiB x 1024 and RS(10,4) 1 MiB x 256:
  (a) data-only random losses of 1..m units per stripe (the masks of bench.py
      --decode-mode mixed): hec_decode_device_mixed against
      hec_reconstruct_device_mixed with the same masks.  The decode call's code
      is unchanged, so it is the yardstick; the margin is the spread of its
      own rounds.
  (b) one lost unit per stripe, index uniform over k+m (a dead DataNode's
      block groups), repaired in place: k reads + 1 write per stripe.
Both are checked against the original cells before anything is timed.
  python3 scripts/probe_reconstruct.py
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
    gib = [nbytes / (t * 1e-3) / 2**30 for t in (med, hi, lo)]
    print(f"{name:18s} {variant:28s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
          f"{gib[0]:.0f} GiB/s [{gib[1]:.0f} .. {gib[2]:.0f}]  {nbytes / (med * 1e-3) / PEAK:.3f} of peak", flush=True)
    print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)


def main():
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for k, m, S in CONFIGS:
        n = k + m
        name = f"RS({k},{m}) x {S}"
        coder = H.Coder(k, m, 0)
        cells = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=g)
        ptrs, strides = H.stripe_layout_ptrs(cells, n)
        coder.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], CELL, S, stream.cuda_stream)
        torch.cuda.synchronize()
        rng = np.random.default_rng(0x5EED_EC00 + k)
        full = (1 << n) - 1

        # (a) data-only losses: decode_device_mixed vs reconstruct_device_mixed
        masks, erased = [], 0
        for _ in range(S):
            e = int(rng.integers(1, m + 1))
            lost = rng.choice(k, size=e, replace=False)
            masks.append(full & ~sum(1 << int(i) for i in lost))
            erased += e
        o_dec = torch.zeros((S, k, CELL), dtype=torch.uint8, device=dev)
        o_rec = torch.zeros((S, k, CELL), dtype=torch.uint8, device=dev)
        dp, ds = H.stripe_layout_ptrs(o_dec, k)
        rp, rs = H.stripe_layout_ptrs(o_rec, k)
        ws_d = torch.empty(coder.decode_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        ws_r = torch.empty(coder.reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

        def dec():
            coder.decode_device_mixed(ptrs, strides, dp, ds, masks, CELL, S, ws_d.data_ptr(), ws_d.numel(),
                                      stream.cuda_stream)

        def rec():
            coder.reconstruct_device_mixed(ptrs, strides, rp + [None] * m, rs + [0] * m, masks, None, CELL, S,
                                           ws_r.data_ptr(), ws_r.numel(), stream.cuda_stream)

        dec()
        rec()
        torch.cuda.synchronize()
        lost_t = torch.tensor([[not (mk >> j) & 1 for j in range(k)] for mk in masks], device=dev)
        assert torch.equal(o_dec, o_rec), name
        assert bool(((o_rec == cells[:, :k]) | ~lost_t[:, :, None]).all()), name
        t_dec, t_rec = [], []
        for _ in range(ROUNDS):
            t_dec.append(timed(stream, dec))
            t_rec.append(timed(stream, rec))
        nbytes = (k * S + erased) * CELL
        report(name, "(a) decode_device_mixed", t_dec, nbytes)
        report(name, "(a) reconstruct_device_mixed", t_rec, nbytes)
        spread = (max(t_dec) - min(t_dec)) / statistics.median(t_dec)
        delta = statistics.median(t_rec) / statistics.median(t_dec) - 1
        print(f"{name:18s} (a) reconstruct vs decode: {delta:+.2%} time; decode's own spread {spread:.2%}", flush=True)
        del o_dec, o_rec

        # (b) one lost unit per stripe, uniform over k+m, repaired in place
        lost_unit = rng.integers(0, n, size=S)
        masks_b = [full & ~(1 << int(u)) for u in lost_unit]
        idx = torch.arange(S, device=dev)
        unit = torch.from_numpy(lost_unit).to(dev)
        saved = cells[idx, unit].clone()
        cells[idx, unit] = 0xEE
        ws_b = torch.empty(coder.reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)

        def repair():
            coder.reconstruct_device_mixed(ptrs, strides, ptrs, strides, masks_b, None, CELL, S, ws_b.data_ptr(),
                                           ws_b.numel(), stream.cuda_stream)

        repair()
        torch.cuda.synchronize()
        assert torch.equal(cells[idx, unit], saved), name
        t_b = [timed(stream, repair) for _ in range(ROUNDS)]
        n_par = int((lost_unit >= k).sum())
        report(name, f"(b) 1 lost unit ({n_par}/{S} parity)", t_b, (k + 1) * S * CELL)
        coder.close()
        del cells, saved
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
