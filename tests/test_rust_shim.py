"""The Rust side of the drop-in (no cargo in this image, so it is checked
as text): the forwarding patch applies to the reference's EC sources, and
the shim's FFI declarations name only functions the C ABI header declares,
at the header's ABI version."""
import os
import re
import subprocess

from conftest import ROOT

PATCH = os.path.join(ROOT, "rust", "patches", "ec_mi355x.patch")
SHIM = os.path.join(ROOT, "rust", "src", "ec", "mi355x.rs")
HEADER = os.path.join(ROOT, "include", "hdfs_ec_amd.h")
PATCHED = {"rust/src/ec/gf256.rs", "rust/src/ec/mod.rs", "rust/benches/ec.rs"}
UNTOUCHED = ("rust/src/hdfs/mod.rs", "rust/src/hdfs/block_writer.rs", "rust/src/hdfs/block_reader.rs")


def _pre_images(patch_text):
    """The lines the patch expects to find, per file: every hunk's context
    and removed lines at the hunk's own line numbers, the lines between the
    hunks (which the patch does not state) filled with placeholders.  A hunk
    whose header disagrees with its body, or that overlaps the one before
    it, fails here."""
    files, cur, ln = {}, None, None
    for line in patch_text.splitlines():
        if line.startswith("--- a/"):
            cur = files.setdefault(line[6:].strip(), [])
            ln = None
        elif line.startswith("+++ "):
            continue
        elif line.startswith("@@"):
            a, na, _, nb = (int(x) for x in re.match(r"@@ -(\d+),(\d+) \+(\d+),(\d+) @@", line).groups())
            assert ln is None or ln == (0, 0), f"hunk before {line} is shorter than its header says"
            assert len(cur) < a, f"{line} overlaps the hunk before it"
            cur.extend(f"// line {i}" for i in range(len(cur) + 1, a))
            ln = (na, nb)
        elif cur is not None and ln is not None:
            old, new = line[:1] in (" ", "-", ""), line[:1] in (" ", "+", "")
            assert old or new, line
            ln = (ln[0] - old, ln[1] - new)
            assert min(ln) >= 0, f"hunk longer than its header says at: {line}"
            if old:
                cur.append(line[1:])
    assert ln == (0, 0), "last hunk is shorter than its header says"
    return {name: "\n".join(lines) + "\n" for name, lines in files.items()}


def _apply_and_check(tree, pristine):
    """Applies the forwarding patch in `tree` (exactly: no fuzz, no offset)
    and checks what it made of the EC sources; `pristine` maps every file's
    path to its text before the patch."""
    r = subprocess.run(["patch", "-p1", "--dry-run", "-i", PATCH], cwd=tree, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["patch", "-p1", "-i", PATCH], cwd=tree, capture_output=True, text=True)
    assert r.returncode == 0
    assert "fuzz" not in r.stdout and "offset" not in r.stdout, r.stdout
    text = (tree / "rust/src/ec/gf256.rs").read_text()
    # Coder::new acquires a pooled engine coder (None -> the reference CPU
    # path, kept unchanged); encode / decode forward to it when present
    assert "gpu: Option<super::mi355x::PooledCoder>" in text
    assert "super::mi355x::PooledCoder::acquire(\"rs\"" in text and ".ok()," in text
    assert text.count("if let Some(gpu) = self.gpu.as_ref()") == 2
    assert '#[cfg(not(feature = "mi355x"))]' not in text  # the CPU bodies stay in both builds
    assert "pub mod mi355x;" in (tree / "rust/src/ec/mod.rs").read_text()
    # the striped writer and reader are the reference's, unchanged: they code
    # one row per Coder call (block_writer.rs:838, ec/mod.rs:71-72) and the
    # engine routes those pageable rows to its host routine -- the 4-row
    # batching of round 4 is gone (measured, the device route
    # lost at both call shapes, and 4 rows bought the host routine +8 % on
    # encode for 4x the writer's buffer)
    for name in UNTOUCHED:
        assert (tree / name).read_text() == pristine[name], name
    # the reference's Criterion bench gains a device-resident group (features
    # benchmark + mi355x) beside its own, which stays as it was: the same
    # 6 x 16 MiB slices, encode and decode 1 / 2 / 3 missing through GpuCoder
    bench = (tree / "rust/benches/ec.rs").read_text()
    ref = pristine["rust/benches/ec.rs"]
    assert bench.startswith(ref[:ref.index("criterion_group!")])
    assert "fn bench_mi355x(c: &mut Criterion)" in bench
    assert 'benchmark_group("rs-encode-mi355x")' in bench and 'benchmark_group("rs-decode-mi355x")' in bench
    assert "coder.encode_device(" in bench and "coder.decode_device(" in bench
    assert "criterion_group!(benches, bench, bench_mi355x);" in bench
    assert '#[cfg(not(feature = "mi355x"))]\ncriterion_group!(benches, bench);' in bench


def test_forwarding_patch_applies_to_reference(tmp_path):
    """Self-contained: the tree the patch is applied to is the one the patch
    itself describes (its hunks' context and removed lines at their line
    numbers).  With $HDFS_NATIVE_REFERENCE naming a checkout of the reference,
    the same patch and checks also run on that checkout's files."""
    patch_text = open(PATCH).read()
    patched = {ln[6:].strip() for ln in patch_text.splitlines() if ln.startswith("+++ b/")}
    assert patched == PATCHED, patched
    pristine = _pre_images(patch_text)
    assert set(pristine) == PATCHED
    for name in UNTOUCHED:
        pristine[name] = f"// {name}: not named by the patch\n"
    tree = tmp_path / "stated"
    for name, text in pristine.items():
        (tree / name).parent.mkdir(parents=True, exist_ok=True)
        (tree / name).write_text(text)
    _apply_and_check(tree, pristine)
    ref_root = os.environ.get("HDFS_NATIVE_REFERENCE")
    if ref_root:
        tree = tmp_path / "checkout"
        names = sorted(PATCHED) + list(UNTOUCHED) + ["rust/src/ec/matrix.rs"]
        pristine = {name: open(os.path.join(ref_root, name)).read() for name in names}
        for name, text in pristine.items():
            (tree / name).parent.mkdir(parents=True, exist_ok=True)
            (tree / name).write_text(text)
        _apply_and_check(tree, pristine)
    assert not os.path.exists(os.path.join(ROOT, "rust", "src", "hdfs", "ec_rows.rs"))


def test_shim_ffi_matches_header():
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hec_[a-z_0-9]+)\s*\(", header))
    shim = open(SHIM).read()
    ffi = shim[shim.index('unsafe extern "C" {'):]
    ffi = ffi[:ffi.index("\n}\n")]
    used = set(re.findall(r"fn (hec_[a-z_0-9]+)\(", ffi))
    assert used and used <= declared, used - declared
    abi = int(re.search(r"#define HEC_ABI_VERSION (\d+)", header).group(1))
    assert f"const ABI_VERSION: c_int = {abi};" in shim
