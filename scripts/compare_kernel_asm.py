#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel.

    compare_kernel_asm.py OLD.s NEW.s [--registers] [--map 'REGEX=REPLACEMENT' ...]

The listings are what `hipcc $(HIPFLAGS) --save-temps -c x.hip` leaves as
x-hip-amdgcn-amd-amdhsa-gfx950.s.  Comments and .file/.ident/.loc lines are
dropped.  A kernel PASSES when its metadata (VGPRs, AGPRs, SGPRs, both spill
counts, private and group segment sizes) is identical and its instruction
lines differ at most in the order of the two sources of a commutative op.
Prints one line per kernel (names through c++filt where there is one);
--registers adds the resource lines, parent and new, of each kernel that
differs.  Each --map rewrites the mangled names of the new listing
(re.sub on every line, in the order given), so that a kernel that was renamed
is paired with the name it had.  Exit status 1 when a kernel differs.
"""
import re
import subprocess
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")
COMMUTATIVE = re.compile(r"^(v|s)_(xor|or|and|add_u32|add_nc_u32|add_co_u32|min_u32|max_u32|mul_lo_u32|mul_hi_u32|"
                         r"xnor|add_i32)(_b32|_b64|_e32|_e64)*$")


def clean(path, maps=()):
    out = []
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
        for pat, repl in maps:
            line = pat.sub(repl, line)
        s = line.strip()
        if not s or s.startswith((".file", ".ident", ".loc")) or "__hip_cuid_" in s:
            continue
        out.append(s)
    return out


def kernels(lines):
    """name -> instruction lines of the function body"""
    body, cur, name = {}, None, None
    for s in lines:
        m = re.match(r"^(_Z\w+):$", s)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                body[name] = cur
                cur = None
            else:
                cur.append(s)
    return body


def metadata(lines):
    """name -> {field: value} from the amdhsa.kernels notes"""
    meta, cur = {}, {}
    for s in lines:
        s = s.lstrip("- ").strip()
        m = re.match(r"^(\.\w+):\s*(.*)$", s)
        if not m:
            continue
        key, val = m.groups()
        if key in META:
            cur[key] = val
        elif key == ".name" and val.startswith("_Z") and key not in cur:
            cur[key] = val
        elif key == ".wavefront_size":  # last field of a kernel's record
            if ".name" in cur:
                meta[cur.pop(".name")] = cur
            cur = {}
    return meta


def same_line(a, b):
    if a == b:
        return True
    pa, pb = a.split(None, 1), b.split(None, 1)
    if len(pa) != 2 or len(pb) != 2 or pa[0] != pb[0] or not COMMUTATIVE.match(pa[0]):
        return False
    oa, ob = [x.strip() for x in pa[1].split(",")], [x.strip() for x in pb[1].split(",")]
    # the destination(s) stay; the last two operands may swap
    return len(oa) == len(ob) >= 3 and oa[:-2] == ob[:-2] and oa[-2:] == ob[-2:][::-1]


def demangled(names):
    """mangled -> 'gf_scrub<6,3,4,256,1>' with c++filt where there is one"""
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, out.split("\n")):
        d = re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)).replace("hec::", "").replace(", ", ",")
        short[n] = d
    return short


def resources(tag, name, m):
    """one line in the format of profiles/scrub_crc/registers.txt"""
    if not m:
        return f"{tag} {name}  (no metadata)"
    waves = min(8, 512 // ((int(m[".vgpr_count"]) + 7) // 8 * 8))
    return (f"{tag} {name}  SGPRs {m['.sgpr_count']}  VGPRs {m['.vgpr_count']}  AGPRs {m['.agpr_count']}  "
            f"scratch {m['.private_segment_fixed_size']} B/lane  LDS {m['.group_segment_fixed_size']} B/block  "
            f"occupancy {waves} waves/SIMD")


def main():
    argv, args, maps = sys.argv[1:], [], []
    while argv:
        a = argv.pop(0)
        if a == "--map":
            pat, repl = argv.pop(0).split("=", 1)
            maps.append((re.compile(pat), repl))
        elif not a.startswith("--"):
            args.append(a)
    regs = "--registers" in sys.argv
    old, new = clean(args[0]), clean(args[1], maps)
    ko, kn = kernels(old), kernels(new)
    mo, mn = metadata(old), metadata(new)
    names = sorted(set(ko) | set(kn))
    short = demangled(names)
    bad = 0
    for name in names:
        if name not in ko or name not in kn:
            print(f"differs  {short[name]}: only in {'old' if name in ko else 'new'}")
            bad += 1
            continue
        a, b = ko[name], kn[name]
        ma, mb = mo.get(name, {}), mn.get(name, {})
        why = []
        if ma != mb:
            why.append("metadata " + " ".join(f"{k[1:]} {ma.get(k)}->{mb.get(k)}" for k in META if ma.get(k) != mb.get(k)))
        if len(a) != len(b):
            why.append(f"{len(a)} -> {len(b)} lines")
        elif any(not same_line(x, y) for x, y in zip(a, b)):
            why.append(f"{sum(not same_line(x, y) for x, y in zip(a, b))} of {len(a)} lines differ")
        if why:
            print(f"differs  {short[name]}: " + "; ".join(why))
            bad += 1
            if regs:
                print("  " + resources("parent", short[name], ma))
                print("  " + resources("new   ", short[name], mb))
        else:
            swaps = sum(x != y for x, y in zip(a, b))
            print(f"pass  {short[name]}: " + (f"{swaps} commutative operand swaps in {len(a)} lines" if swaps
                                              else f"identical ({len(a)} lines)"))
    print(f"{len(ko)} kernels old, {len(kn)} new, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
