"""Measurement probe (GPU box): the degraded scrub (hec_scrub_device_mixed,
kernel gf_scrub_mixed) on one MI355X, product library, one process, the same
device buffers, rounds alternated, HIP events around REPS back-to-back calls
after a warm call; each config first runs WARM_CALLS untimed calls on its
buffers.  Per config, RS(6,3) and RS(10,4), 1 MiB cells x 256 stripes:
  (a) all-present masks through the mixed call, against hec_scrub_device on the
      same batch (both read (k+m) * cell_len per stripe); time per byte read.
  (b) one unit missing per stripe, the index uniform over k+m, clean; against
      the same hec_scrub_device rounds per byte read ((k+m-1) cells per stripe)
      and against what a caller composes today: hec_reconstruct_device_mixed of
      the extras into scratch (present = the survivors only, want = the extras)
      and a torch compare per stripe.  The gate: the mixed scrub's median is
      shorter than the composition's median minus the composition's own
      round-to-round spread.
  (c) as (b) with one corrupt byte in 1 % of the stripes: the slow path.
Every result is checked before anything is timed (clean: all zero; dirty: the
corrupt stripes located, nothing else).
  python3 scripts/probe_scrub_mixed.py
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))

CELL = int(os.environ.get("PROBE_CELL", str(1 << 20)))
STRIPES = int(os.environ.get("PROBE_STRIPES", "256"))
CONFIGS = [(6, 3), (10, 4)]
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "5"))
REPS = int(os.environ.get("PROBE_REPS", "20"))
WARM_CALLS = int(os.environ.get("PROBE_WARM_CALLS", "200"))  # per config, before anything is timed
PEAK = 8e12  # HBM bytes/s


def main():
    import numpy as np
    import torch

    import hdfs_native_ec as H

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(23)

    def timed(fn):
        fn()  # warm
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(REPS):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / REPS

    def report(name, variant, ts, nbytes):
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        print(f"{name:16s} {variant:46s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
              f"{nbytes / (med * 1e-3) / 2**30:.0f} GiB/s read  {nbytes / (med * 1e-3) / PEAK:.3f} of peak", flush=True)
        print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)
        return med

    for k, m in CONFIGS:
        n, S = k + m, STRIPES
        full = (1 << n) - 1
        name = f"RS({k},{m}) x {S}"
        coder = H.Coder(k, m, 0)
        cells = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=g)
        ptrs, strides = H.stripe_layout_ptrs(cells, n)
        coder.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], CELL, S, stream.cuda_stream)
        res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        ws = torch.empty(coder.scrub_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        rng = np.random.default_rng(0x5C2C + k)
        lost = [int(t) for t in rng.integers(0, n, size=S)]
        masks_full = [full] * S
        masks_loss = [full & ~(1 << t) for t in lost]

        def scrub():
            coder.scrub_device(ptrs, strides, CELL, S, res.data_ptr(), stream.cuda_stream)

        def mixed(masks):
            coder.scrub_device_mixed(ptrs, strides, masks, CELL, S, res.data_ptr(), ws.data_ptr(), ws.numel(),
                                     stream.cuda_stream)

        # the composition: rebuild the e extras of every stripe from its k
        # survivors into scratch (in the extras' own slots of a second image),
        # then compare with the stored extras
        scratch = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
        sp, ss = H.stripe_layout_ptrs(scratch, n)
        rws = torch.empty(max(coder.reconstruct_mixed_workspace_size(S), 1), dtype=torch.uint8, device=dev)
        surv_masks, extra_masks = [], []
        for mask in masks_loss:
            pres = [i for i in range(n) if (mask >> i) & 1]
            surv_masks.append(sum(1 << i for i in pres[:k]))
            extra_masks.append(sum(1 << i for i in pres[k:]))
        # the compare reads the rebuilt and the stored extras only: their rows
        # of the two images, gathered (e = m - 1 rows per stripe)
        rows = torch.tensor([s_ * n + i for s_, em in enumerate(extra_masks) for i in range(n) if (em >> i) & 1],
                            dtype=torch.int64, device=dev)
        flags = []

        def composed():
            coder.reconstruct_device_mixed(ptrs, strides, sp, ss, surv_masks, extra_masks, CELL, S, rws.data_ptr(),
                                           rws.numel(), stream.cuda_stream)
            rebuilt = scratch.view(S * n, CELL).index_select(0, rows)
            stored = cells.view(S * n, CELL).index_select(0, rows)
            flags.append((rebuilt != stored).view(S, -1).any(dim=1))
            del flags[:-1]

        def check(fn, expect):
            res.fill_(-1)
            fn()
            torch.cuda.synchronize()
            got = {s: (int(r), int(b)) for s, (r, b) in enumerate(res.cpu().tolist()) if (r, b) != (0, 0)}
            assert set(got) == set(expect), (name, sorted(got), sorted(expect))
            for s, unit in expect.items():
                assert H.scrub_verdict(*got[s], n) == (H.HEC_SCRUB_LOCATED, unit), (name, s, got[s])

        check(scrub, {})
        check(lambda: mixed(masks_full), {})
        check(lambda: mixed(masks_loss), {})
        composed()
        torch.cuda.synchronize()
        assert not bool(flags[-1].any()), name
        for _ in range(WARM_CALLS // 4):
            scrub()
            mixed(masks_full)
            mixed(masks_loss)
            composed()
        torch.cuda.synchronize()

        # (c)'s corruption: one byte of a present unit in 1 % of the stripes
        dirty = sorted(int(s) for s in rng.choice(S, size=max(1, S // 100), replace=False))
        units = {s: [i for i in range(n) if i != lost[s]][int(rng.integers(0, n - 1))] for s in dirty}
        where = {s: int(rng.integers(0, CELL)) for s in dirty}

        def toggle():
            for s, u in units.items():
                cells[s, u, where[s]] ^= 0x40

        toggle()
        check(lambda: mixed(masks_loss), units)
        toggle()
        check(lambda: mixed(masks_loss), {})

        t = {v: [] for v in ("uniform", "a", "b", "c", "composed")}
        for _ in range(ROUNDS):
            t["uniform"].append(timed(scrub))
            t["a"].append(timed(lambda: mixed(masks_full)))
            t["b"].append(timed(lambda: mixed(masks_loss)))
            toggle()
            t["c"].append(timed(lambda: mixed(masks_loss)))
            toggle()
            t["composed"].append(timed(composed))
        check(lambda: mixed(masks_loss), {})
        all_b, loss_b = n * S * CELL, (n - 1) * S * CELL
        uni = report(name, "hec_scrub_device, all present", t["uniform"], all_b)
        a = report(name, "(a) mixed, all-present masks", t["a"], all_b)
        b = report(name, "(b) mixed, one unit missing per stripe", t["b"], loss_b)
        c = report(name, f"(c) as (b), one corrupt byte in {len(dirty)} stripes", t["c"], loss_b)
        # the rate shown for the composition counts the k survivor cells its reconstruction reads
        comp = report(name, "(b) composed: reconstruct extras + torch compare", t["composed"], k * S * CELL)
        spread_u = (max(t["uniform"]) - min(t["uniform"])) / uni
        spread_c = max(t["composed"]) - min(t["composed"])
        print(f"{name:16s} (a) time per byte read, mixed / uniform: {a / uni:.4f} (uniform's own spread {spread_u:.2%})")
        print(f"{name:16s} (b) time per byte read, mixed / uniform: {(b / loss_b) / (uni / all_b):.4f}")
        print(f"{name:16s} (c) / (b): {c / b:.4f}")
        gate = b < comp - spread_c
        print(f"{name:16s} gate: (b) {b:.4f} ms < composed {comp:.4f} ms - its spread {spread_c:.4f} ms: "
              f"{'PASS' if gate else 'FAIL'} ({comp / b:.2f}x); scratch {n * S * CELL >> 20} MiB + torch's temporaries", flush=True)
        coder.close()
        del cells, scratch, flags, ws, rws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
