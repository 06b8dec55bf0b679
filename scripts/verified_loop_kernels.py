#!/usr/bin/env python3
"""Checks a kernel trace of tests/test_gpu_verified_loops.py against the grids
that tests/verified_loop_cases.py restates from the launchers: every kernel
family must have run on its default grid (blocks_per_cu x CUs, which the
launchers clamp to the tile count, so the cap appears only where a launch had
more tiles than that) and, with the measurement build, on 1 and 5 blocks.

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python -m pytest tests/test_gpu_verified_loops.py
    scripts/verified_loop_kernels.py OUT/.../run_kernel_trace.csv CUS [kernels.txt]

Prints one line per family (the cap, whether it was seen, the largest grid seen,
the small grids seen); with a third argument, writes the distinct kernel names
with their grid sizes in blocks and the launches of each there.  Exit status 1
if a family never ran on its cap or ran on a larger grid."""
import collections
import csv
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import verified_loop_cases as L  # noqa: E402

# (family, with a stripe list) -> what its kernel names match
FAMILY = (
    ("recon", re.compile(r"gf_reconstruct_crc<\d+, \d+, \d+, \d+, (true|false), true>")),
    ("sums", re.compile(r"gf_reconstruct_crc<\d+, \d+, \d+, \d+, (true|false), false>")),
    ("scrub", re.compile(r"gf_scrub_crc<")),
    ("repair_rows", re.compile(r"gf_crc_rows<hec::RowsRepair<")),
    ("encode_rows", re.compile(r"gf_crc_rows<hec::RowsEncode,")),
    ("scrub_rows", re.compile(r"gf_scrub_crc_rows<")),
    ("read_rows", re.compile(r"gf_read_rows<")),
)
BYTES = re.compile(r"gf_(reconstruct_sums|reconstruct_rows|encode_rows|read_rows|scrub_rows)_bytes<")


def main():
    cus = int(sys.argv[2])
    grids = collections.Counter()  # (name, blocks) -> launches
    with open(sys.argv[1], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "hec::" not in name and not name.startswith("gf_"):
                continue
            grid = int(r.get("Grid_Size_X") or r["Grid_Size"])
            block = int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
            grids[(name, grid // block)] += 1
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write("launches  blocks  kernel\n")
            for (name, blocks), launches in sorted(grids.items()):
                f.write("%8d  %6d  %s\n" % (launches, blocks, name))
    bad = 0
    for family, pattern in FAMILY:
        seen = sorted({blocks for (name, blocks) in grids if pattern.search(name)})
        caps = [L.blocks_per_cu(family) * cus]
        if family == "scrub":
            caps.append(L.blocks_per_cu(family, with_list=True) * cus)
        if family == "scrub_rows":  # without a list the kernel gets one stripe, the short last one
            caps = [L.blocks_per_cu(family, with_list=True) * cus]
        ok = all(c in seen for c in caps) and (not seen or max(seen) <= max(caps))
        print("%-12s caps %-12s seen %-5s largest %6d  of 1 and 5 blocks seen: %s" % (
            family, "/".join(map(str, caps)), "yes" if ok else "NO", max(seen) if seen else 0,
            [g for g in L.BLOCK_GRIDS if g in seen]))
        bad += not ok
    cap = L.byte_lanes(cus) // 256
    names = sorted({BYTES.search(name).group(0) for (name, _) in grids if BYTES.search(name)})
    for kernel in names:
        seen = sorted({blocks for (name, blocks) in grids if kernel in name})
        ok = cap in seen and max(seen) <= cap
        print("%-34s cap %6d  seen %-3s largest %6d" % (kernel + ">", cap, "yes" if ok else "NO", max(seen)))
        bad += not ok
    print("byte-wise kernels in the trace: %d of 5" % len({n.split("<")[0] for n in names}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
