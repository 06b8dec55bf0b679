"""Measurement probe (GPU box): host time to queue a verified mixed call, that
is the wall clock around CALLS back-to-back calls with no synchronise inside
(the stream is drained between rounds, outside the clock).  Small cells, so
that the device keeps up and the figure is the host's: planning, the workspace
image, filling the argument blocks and the launches themselves, plus the
Python wrapper, which is the same for every library.

RS(6,3) and RS(10,4), 64 stripes of 4 KiB cells, one unit lost per stripe
(cycling over all units, so k + m plans per call), CRC32C per 512-B chunk, with
d_expected:
  full   hec_reconstruct_crc_device_mixed, every stripe full
  rows   hec_reconstruct_crc_rows_device_mixed, every second stripe short
HEC_LIB_PATH picks the library (profiles/mixed_planner/README.md).
  python3 scripts/probe_capi_host.py
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hdfs-native_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import ec_oracle  # noqa: E402
from probe_reconstruct_crc_rows import BPC, Batch  # noqa: E402

CELL, STRIPES = 4096, 64
CALLS = int(os.environ.get("PROBE_CALLS", "20"))
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "40"))


def host_us(fn):
    fn()  # warm: code objects, plan cache, staging
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        ts.append((time.perf_counter() - t0) / CALLS * 1e6)
        torch.cuda.synchronize()
    return ts


def main():
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    clib = ec_oracle.load_c_oracle()
    for k, m in ((6, 3), (10, 4)):
        n, full = k + m, k * CELL
        lost = [s % n for s in range(STRIPES)]
        rs = [full if s % 2 == 0 else 1 + (s * 2654435761) % (full - 1) for s in range(STRIPES)]
        for name, b, fn in (("full", Batch(dev, gen, clib, k, m, STRIPES, CELL, BPC, [full] * STRIPES, lost), "yard"),
                            ("rows", Batch(dev, gen, clib, k, m, STRIPES, CELL, BPC, rs, lost), "new")):
            getattr(b, fn)(True, st)
            b.check(f"RS({k},{m}) {name}")
            ts = host_us(lambda: getattr(b, fn)(True, st))
            print(f"RS({k},{m}) x {STRIPES} {name}: median {statistics.median(ts):.2f} us per call "
                  f"[{min(ts):.2f} .. {max(ts):.2f}] over {ROUNDS} rounds of {CALLS} calls", flush=True)


if __name__ == "__main__":
    main()
