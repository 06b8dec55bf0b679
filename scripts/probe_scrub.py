"""Measurement probe (GPU box): the stripe scrub (hec_scrub_device, kernel
gf_scrub) on one MI355X, product library, one process, the same device
buffers, rounds alternated, HIP events around REPS back-to-back calls after a
warm call; each config first runs WARM_CALLS untimed calls on its buffers.
Per config, RS(6,3) and RS(10,4), 1 MiB cells x 256 stripes:
  (1) a clean batch: hec_scrub_device against hec_encode_device of the same
      batch (into scratch parity).  Both move (k+m) * cell_len per stripe, so
      the encode call is the yardstick and the margin is the spread of its own
      rounds.
  (2) the same batch with one corrupt byte in 1 % of the stripes, and with one
      wholly random unit in 1 % of the stripes: the cost of the slow path.
  (3) what a caller composes today: encode into scratch, then a torch compare
      with the stored parity (one mismatch flag per stripe).
Every scrub result is checked (clean: all zero; dirty: the corrupt stripes and
units, nothing else) before anything is timed.
  python3 scripts/probe_scrub.py
Kernel times: run the same command under `rocprofv3 --kernel-trace` with
PROBE_SCHEDULE=FILE (the probe writes the order of its launches there), then
  python3 scripts/probe_scrub.py --summarize TRACE_CSV FILE
"""
import csv
import json
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
PEAK = 8e12  # HBM bytes/s

schedule = []  # one entry per engine launch, in order: [kernel kind, phase, timed]


def summarize(trace_csv, schedule_json):
    """Kernel durations of a rocprofv3 kernel trace of this probe, per phase."""
    sched = json.load(open(schedule_json))
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    names = {"scrub": "gf_scrub<", "encode": "gf_matmul_v16<"}
    for kind, needle in names.items():
        got = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if needle in r["Kernel_Name"]]
        want = [s for s in sched if s[0] == kind]
        assert len(got) == len(want), (kind, len(got), len(want))
        phases = {}
        for us, (_, phase, is_timed) in zip(got, want):
            if is_timed:
                phases.setdefault(phase, []).append(us)
        for phase, v in phases.items():
            print(f"{kind:7s} {phase:34s} n {len(v):3d}  median {statistics.median(v):8.1f} us  "
                  f"[{min(v):.1f} .. {max(v):.1f}]")


def main():
    import numpy as np
    import torch

    import hdfs_native_ec as H

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(17)

    def timed(fn, kind, phase):
        fn()  # warm: code objects, counter sets
        schedule.append([kind, phase, False])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(REPS):
            fn()
            schedule.append([kind, phase, True])
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / REPS

    def report(name, variant, ts, nbytes):
        med, lo, hi = statistics.median(ts), min(ts), max(ts)
        print(f"{name:16s} {variant:40s} median {med:.4f} ms  [{lo:.4f} .. {hi:.4f}]  "
              f"{nbytes / (med * 1e-3) / 2**30:.0f} GiB/s  {nbytes / (med * 1e-3) / PEAK:.3f} of peak", flush=True)
        print("  raw ms: " + " ".join(f"{t:.4f}" for t in ts), flush=True)

    for k, m in CONFIGS:
        n, S = k + m, STRIPES
        name = f"RS({k},{m}) x {S}"
        coder = H.Coder(k, m, 0)
        cells = torch.empty((S, n, CELL), dtype=torch.uint8, device=dev)
        cells.random_(0, 256, generator=g)
        ptrs, strides = H.stripe_layout_ptrs(cells, n)
        coder.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], CELL, S, stream.cuda_stream)
        schedule.append(["encode", f"{name} setup", False])
        scratch = torch.empty((S, m, CELL), dtype=torch.uint8, device=dev)
        sp, ss = H.stripe_layout_ptrs(scratch, m)
        res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        nbytes = n * S * CELL

        def enc():
            coder.encode_device(ptrs[:k], strides[:k], sp, ss, CELL, S, stream.cuda_stream)

        def scrub():
            coder.scrub_device(ptrs, strides, CELL, S, res.data_ptr(), stream.cuda_stream)

        def checked(phase, expect):
            scrub()
            schedule.append(["scrub", phase, False])
            torch.cuda.synchronize()
            got = {s: (int(r), int(b)) for s, (r, b) in enumerate(res.cpu().tolist()) if (r, b) != (0, 0)}
            assert set(got) == set(expect), (name, phase, sorted(got), sorted(expect))
            for s, unit in expect.items():
                assert H.scrub_verdict(*got[s], n) == (H.HEC_SCRUB_LOCATED, unit), (name, phase, s, got[s])
            return got

        # (1) clean: encode vs scrub, alternated
        p1 = f"{name} (1) clean"
        checked(p1, {})
        # a fresh process's first tens of milliseconds on new buffers run slow
        # (every phase's rounds fell by 10-20 % without this): reach steady
        # state on these buffers first
        for _ in range(WARM_CALLS // 2):
            enc()
            schedule.append(["encode", p1, False])
            scrub()
            schedule.append(["scrub", p1, False])
        torch.cuda.synchronize()
        t_enc, t_scr = [], []
        for _ in range(ROUNDS):
            t_enc.append(timed(enc, "encode", p1))
            t_scr.append(timed(scrub, "scrub", p1))
        assert torch.equal(scratch, cells[:, k:]), name
        report(name, "(1) hec_encode_device (scratch parity)", t_enc, nbytes)
        report(name, "(1) hec_scrub_device, clean", t_scr, nbytes)
        spread = (max(t_enc) - min(t_enc)) / statistics.median(t_enc)
        ratio = statistics.median(t_scr) / statistics.median(t_enc)
        print(f"{name:16s} (1) scrub / encode time {ratio:.4f}; encode's own spread {spread:.2%}", flush=True)

        # (2) 1 % of the stripes dirty: one byte, or one wholly random unit.  The
        # three states of the batch are toggled in place between rounds and
        # timed in turn (clean, one byte, one unit; clean, ...), so that a drift
        # of the box over the phase reaches all three alike
        rng = np.random.default_rng(0x5C2B + k)
        dirty = sorted(int(s) for s in rng.choice(S, size=max(1, S // 100), replace=False))
        units = {s: int(rng.integers(0, n)) for s in dirty}
        saved = {s: cells[s, u].clone() for s, u in units.items()}
        where = {s: int(rng.integers(0, CELL)) for s in dirty}
        garbage = {s: torch.empty(CELL, dtype=torch.uint8, device=dev).random_(0, 256, generator=g) for s in dirty}
        variants = ("clean", "one corrupt byte", "one random unit")

        def set_state(variant):
            for s, u in units.items():
                cells[s, u] = garbage[s] if variant == "one random unit" else saved[s]
                if variant == "one corrupt byte":
                    cells[s, u, where[s]] ^= 0x40

        for variant in variants[1:]:
            set_state(variant)
            got = checked(f"{name} (2) check", units)
            if variant == "one corrupt byte":
                assert all(b == 1 for _, b in got.values()), got
        t2 = {v: [] for v in variants}
        for _ in range(ROUNDS):
            for variant in variants:
                set_state(variant)
                t2[variant].append(timed(scrub, "scrub", f"{name} (2) {variant}"))
        for variant in variants:
            report(name, f"(2) scrub, {variant}" + ("" if variant == "clean" else f" in {len(dirty)} stripes"),
                   t2[variant], nbytes)
        spread2 = (max(t2["clean"]) - min(t2["clean"])) / statistics.median(t2["clean"])
        for variant in variants[1:]:
            print(f"{name:16s} (2) {variant}: {statistics.median(t2[variant]) / statistics.median(t2['clean']):.4f} "
                  f"of the clean scrub beside it (whose own spread is {spread2:.2%})", flush=True)
        set_state("clean")
        checked(f"{name} restored", {})

        # (3) the composed alternative: encode into scratch + a torch compare per stripe
        stored = cells[:, k:]
        flags = []

        def composed():
            enc()
            flags.append((scratch != stored).flatten(1).any(dim=1))
            del flags[:-1]

        p3 = f"{name} (3) composed"
        t_cmp = [timed(composed, "encode", p3) for _ in range(ROUNDS)]
        assert not bool(flags[-1].any()), name
        report(name, "(3) encode to scratch + torch compare", t_cmp, (n + 2 * m) * S * CELL)
        print(f"{name:16s} (3) composed / scrub time {statistics.median(t_cmp) / statistics.median(t_scr):.2f}x; "
              f"scratch {m * S * CELL >> 20} MiB (+ torch's {m * S * CELL >> 20} MiB of flags per compare)", flush=True)
        coder.close()
        del cells, scratch, stored, saved, garbage, flags
        torch.cuda.empty_cache()
    if os.environ.get("PROBE_SCHEDULE"):
        json.dump(schedule, open(os.environ["PROBE_SCHEDULE"], "w"))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        main()
