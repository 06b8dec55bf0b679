#!/usr/bin/env python3
"""Checks a kernel trace of tests/test_gpu_rows_shapes.py against the lists of
tests/rows_shape_cases.py: every listed instantiation of the short-stripe
register kernels must have been launched.

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python -m pytest tests/test_gpu_rows_shapes.py
    scripts/rows_shape_kernels.py OUT/.../run_kernel_stats.csv [kernels.txt]

Prints one line per kernel family (listed, seen, missing) and the names that
are missing; with a second argument, writes the distinct names of the project's
kernels in the trace (one per line, with the number of launches) there.  Exit
status 1 if an instantiation is missing."""
import csv
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import rows_shape_cases as C  # noqa: E402


def main():
    with open(sys.argv[1], newline="") as f:
        rows = [(r["Name"], int(r["Calls"])) for r in csv.DictReader(f)]
    ours = sorted((name, calls) for name, calls in rows if "hec::" in name or name.startswith("gf_"))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            for name, calls in ours:
                f.write("%6d  %s\n" % (calls, name))
    missing = 0
    for family, shapes in (("repair", C.REPAIR_SHAPES), ("encode", C.ENCODE_SHAPES), ("scrub", C.SCRUB_SHAPES),
                           ("read", C.READ_SHAPES)):
        want = {C.kernel_name(s): s for s in shapes}
        seen = {w for w in want if any(w + "(" in name or name.endswith(w) for name, _ in ours)}
        print("%-6s listed %2d  seen %2d  missing %2d" % (family, len(want), len(seen), len(want) - len(seen)))
        for w in sorted(set(want) - seen):
            print("    missing:", w, tuple(want[w]))
        missing += len(want) - len(seen)
    byte_route = [(name, calls) for name, calls in ours if "_rows_bytes" in name]
    print("byte-wise route kernels in the trace:", byte_route or "none")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
