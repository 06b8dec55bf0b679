#!/usr/bin/env python3
"""Checks kernel traces of tests/test_gpu_fused_launch.py and of its child
tests/fused_generic_child.py against the lists of tests/fused_launch_cases.py:
every instantiation of gf_fused_crc the cases name must have been launched.

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python -m pytest tests/test_gpu_fused_launch.py
    rocprofv3 --kernel-trace --stats -d OUT -o child --output-format csv -- \\
        env HEC_JIT=0 python tests/fused_generic_child.py
    scripts/fused_launch_kernels.py kernels.txt OUT/.../run_kernel_stats.csv OUT/.../child_kernel_stats.csv

Writes the distinct gf_fused_crc<...> names of all the traces (launches and
name, one per line) to the first argument and prints one line per family
(listed, seen, missing).  Exit status 1 if an instantiation is missing."""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import fused_launch_cases as C  # noqa: E402

# <K, R, SLABS, SCHEME, KIND, VERIFY, WPE, PAIR, NET, PFD, WQ>
NAME = re.compile(r"gf_fused_crc<(\d+), (\d+), (\d+), (\d+), (\d+), (true|false), (\d+), (true|false), (.+?), (\d+)"
                  r"(?:, (true|false))?>\(")


def net_of(text):
    return "RsNet" if "RsNet" in text else "Net" if "jit_plan" in text else "PermNet"


def main():
    seen = {}
    for path in sys.argv[2:]:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "gf_fused_crc<" in r["Name"]:
                    seen[r["Name"]] = seen.get(r["Name"], 0) + int(r["Calls"])
    with open(sys.argv[1], "w") as f:
        for name in sorted(seen):
            f.write("%6d  %s\n" % (seen[name], name))
    kernels = set()  # (K, R, KIND, verify, net, queue)
    for name in seen:
        m = NAME.search(name)
        assert m, name
        kernels.add((int(m.group(1)), int(m.group(2)), int(m.group(5)), m.group(6) == "true", net_of(m.group(9)),
                     m.group(11) == "true"))
    encode = {(k, r) for k, r, _, verify, _, _ in kernels if not verify}
    both = {(k, r) for k, r in ((3, 2), (6, 3), (10, 4))
            if {net for kk, rr, _, v, net, _ in kernels if (kk, rr, v) == (k, r, False)} >= {"PermNet", "RsNet"}}
    queue_encode = {(k, r) for k, r, _, verify, _, q in kernels if not verify and q}
    generic = {(k, r, kind) for k, r, kind, verify, net, _ in kernels if verify and net == "PermNet"}
    special = {(k, r, kind) for k, r, kind, verify, net, _ in kernels if verify and net == "Net"}
    queue_special = {(k, r, kind) for k, r, kind, verify, net, q in kernels if verify and net == "Net" and q}
    kind = {C.CRC32C: 0, C.CRC32: 1}
    families = (
        ("encode (K, R)", {(c.k, c.m) for c in C.encode_cases()}, encode),
        ("encode PermNet and RsNet", {(3, 2), (6, 3), (10, 4)}, both),
        ("encode work queue", {(3, 2), (10, 4)}, queue_encode),
        ("generic verify (K, E, KIND)", {(c.k, c.e, kind[c.ctype]) for c in C.generic_cases()}, generic),
        ("specialised verify (K, E, KIND)", {(c.k, c.e, kind[c.ctype]) for c in C.specialised_cases()}, special),
        ("specialised verify work queue", {(c.k, c.e, kind[c.ctype]) for c in C.specialised_cases()}, queue_special),
    )
    missing = 0
    for family, want, got in families:
        print("%-34s listed %2d  seen %2d  missing %2d" % (family, len(want), len(want & got), len(want - got)))
        for w in sorted(want - got):
            print("    missing:", w)
        missing += len(want - got)
    print("generic verify shapes no caller can reach (E > K), compiled and never launched:", list(C.UNREACHABLE))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
