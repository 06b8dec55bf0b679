"""Measurement probe (GPU box): scrub correction (hec_scrub_correct_device,
kernel gf_scrub_correct) on one MI355X, product library, one process, the same
device buffers, rounds alternated, HIP events; each config first runs
WARM_CALLS untimed calls on its buffers.  Per config, RS(6,3) and RS(10,4),
1 MiB cells x 256 stripes:
  (a) a clean batch: hec_scrub_correct_device alone (REPS back-to-back calls
      over the results of one scrub) beside hec_scrub_device of the same batch.
  (b) 1 % of the stripes with one wholly random unit.  Per timed iteration the
      units are corrupted again on the stream (the same copies in both loops),
      then
        new loop:     scrub, correct, scrub -- nothing leaves the stream; one
                      read-back of the units and the final results afterwards;
        today's loop: scrub, results copied to the host, hec_scrub_verdict per
                      stripe, hec_reconstruct_device_mixed in place (workspace
                      kept across iterations), scrub.
      Events sit around each iteration (the host part of today's loop is inside).
Every output is checked before anything is timed: units, the cells against the
truth, the second scrub all zero.
  python3 scripts/probe_scrub_correct.py
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
WARM_CALLS = int(os.environ.get("PROBE_WARM_CALLS", "400"))  # per config, before anything is timed


def main():
    import numpy as np
    import torch

    import hdfs_native_ec as H

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(23)

    def timed(fn, reps=REPS):
        """ms per call of `reps` back-to-back calls after a warm one."""
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def report(name, variant, ts):
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        print(f"{name:16s} {variant:46s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
              f"spread {(hi - lo) / med:.2%}", flush=True)
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
        truth = cells.clone()
        res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        res2 = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        units = torch.full((S,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        workspace = torch.empty(max(coder.reconstruct_mixed_workspace_size(S), 1), dtype=torch.uint8, device=dev)

        def scrub(into=res):
            coder.scrub_device(ptrs, strides, CELL, S, into.data_ptr(), stream.cuda_stream)

        def correct():
            coder.scrub_correct_device(ptrs, strides, CELL, S, res.data_ptr(), units.data_ptr(), stream.cuda_stream)

        # (a) clean
        scrub()
        correct()
        torch.cuda.synchronize()
        assert not res.any() and (units == H.CORRECT_CLEAN).all() and torch.equal(cells, truth), name
        for _ in range(WARM_CALLS // 2):
            scrub()
            correct()
        torch.cuda.synchronize()
        t_scr, t_cor = [], []
        for _ in range(ROUNDS):
            t_scr.append(timed(scrub))
            t_cor.append(timed(correct))
        ms = report(name, "(a) hec_scrub_device, clean", t_scr)
        mc = report(name, "(a) hec_scrub_correct_device, clean", t_cor)
        print(f"{name:16s} (a) correct / scrub time {mc / ms:.4f}", flush=True)

        # (b) 1 % of the stripes with one random unit
        rng = np.random.default_rng(0x5C2C + k)
        dirty = sorted(int(s) for s in rng.choice(S, size=max(1, S // 100), replace=False))
        hit = {s: int(rng.integers(0, n)) for s in dirty}
        garbage = {s: torch.empty(CELL, dtype=torch.uint8, device=dev).random_(0, 256, generator=g) for s in dirty}
        want_units = [hit.get(s, H.CORRECT_CLEAN) for s in range(S)]

        def corrupt():
            for s, u in hit.items():
                cells[s, u] = garbage[s]

        def new_loop():
            corrupt()
            scrub()
            correct()
            scrub(res2)

        def todays_loop():
            corrupt()
            scrub()
            masks = []
            for ruled, bad in res.cpu().tolist():  # synchronises
                verdict, unit = H.scrub_verdict(ruled & 0xFFFFFFFFFFFFFFFF, bad, n)
                masks.append(full & ~(1 << unit) if verdict == H.HEC_SCRUB_LOCATED else full)
            H.reconstruct_batch_mixed(coder, cells, masks, workspace=workspace)
            scrub(res2)

        for loop in (new_loop, todays_loop):
            units.fill_(0x7F7F7F7F)
            res2.fill_(-1)
            loop()
            torch.cuda.synchronize()
            assert torch.equal(cells, truth) and not res2.any(), (name, loop.__name__)
            assert sorted(s for s, (_, b) in enumerate(res.cpu().tolist()) if b) == dirty, (name, loop.__name__)
            if loop is new_loop:
                assert units.cpu().tolist() == want_units, name
        for _ in range(WARM_CALLS // 8):
            new_loop()
            todays_loop()
        torch.cuda.synchronize()
        t_new, t_old, t_base = [], [], []
        for _ in range(ROUNDS):
            t_new.append(timed(new_loop, max(REPS // 2, 1)))
            t_old.append(timed(todays_loop, max(REPS // 2, 1)))
            t_base.append(timed(lambda: (corrupt(), scrub(), scrub(res2)), max(REPS // 2, 1)))
        mn = report(name, f"(b) scrub, correct, scrub; {len(dirty)} dirty stripes", t_new)
        mo = report(name, "(b) scrub, host verdicts, reconstruct_mixed, scrub", t_old)
        mb = report(name, "(b) the two scrubs and the re-corruption alone", t_base)
        print(f"{name:16s} (b) new / today's loop {mn / mo:.4f}; correction step {mn - mb:.4f} ms against "
              f"{mo - mb:.4f} ms", flush=True)
        coder.close()
        del cells, truth, garbage, workspace
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
