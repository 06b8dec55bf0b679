"""Every compiled instantiation of the short-stripe register kernels on the GPU:
the 64 of the repair (gf_crc_rows<RowsRepair>), the 32 of the encode
(gf_crc_rows<RowsEncode>), the 32 of the scrub (gf_scrub_crc_rows) and the 51 of
the read (gf_read_rows), as rows_shape_cases.py lists them with the code and the
call arguments that reach each.  The other rows tests run RS(6,3), RS(3,2),
RS(10,4) and RS(2,1) only, so most (K, rows) pairs, every K <= 6 kernel with
four rows (the only ones with 4 KiB per wave-tile there) and the odd pairing of
K = 3 never ran.

Each shape runs the uniform form (S = 3 with a short last stripe, one call per
length of rows_shape_cases.shape_lengths) and the mixed form (12 stripes, one
length each).  The cell of 9232 bytes is two wave-tiles at 8 KiB and three at
4 KiB.  Ground truth is the CPU oracle and the images are whole, as in
test_gpu_reconstruct_crc_rows.py (Case), test_gpu_encode_crc_rows.py (Enc),
test_gpu_scrub_crc_rows.py (Batch) and test_gpu_read_crc_rows.py (ReadCase).

A launcher that fell back to the byte-wise route would leave every image exact:
which kernels these tests launch is recorded in profiles/rows_shape_tests."""
import pytest

import hdfs_native_ec as H
import rows_shape_cases as P
from test_gpu_encode_crc_rows import Enc
from test_gpu_read_crc_rows import ReadCase
from test_gpu_reconstruct_crc import coder, present_mask
from test_gpu_reconstruct_crc_rows import Case
from test_gpu_scrub_crc_rows import Batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CT = {"crc32c": H.CHECKSUM_CRC32C, "crc32": H.CHECKSUM_CRC32}
CELL = P.SHAPE_CELL
S_UNIFORM = P.SHAPE_UNIFORM_STRIPES
GUARD = 0xC3
BAND = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def banded(nbytes, dev):
    buf = torch.full((nbytes + 2 * BAND,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[BAND:BAND + nbytes]


def bands_intact(buf, nbytes):
    return bool((buf[:BAND] == GUARD).all()) and bool((buf[BAND + nbytes:] == GUARD).all())


def mixed_lengths(k):
    """(stripe_bytes as passed, the true lengths)."""
    rs = P.mixed_shape_lengths(k)
    return rs, [r or k * CELL for r in rs]


# ---- repair ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.REPAIR_SHAPES, ids=P.shape_id)
def test_repair_shape(dev, shape):
    """RS(k,4), shape.r wanted units: the lost units nearest the cut, a set
    with a parity target and a want subset of a larger loss."""
    k, m, full = shape.k, shape.m, shape.k * CELL
    cod, ctype = coder(k, m), CT[shape.kind]
    modes = ("sep", "same") if shape.verify else (None,)
    runs = []
    for li, r in enumerate(P.shape_lengths(k)):
        rs = [full] * (S_UNIFORM - 1) + [r]
        for ti, (lost, want) in enumerate(P.repair_targets(k, m, shape.r, P.cut_unit(CELL, r))):
            c = Case(cod, k, m, CELL, rs, [lost] * S_UNIFORM, dev, wants=None if want == lost else [want] * S_UNIFORM,
                     expected=modes[(li + ti) % len(modes)], separate=(li + ti) % 2 == 0, pad=(0, 48)[li % 2],
                     ctype=ctype)
            c.uniform()
            runs.append((("uniform", r, lost, want), c))
    sb, true_rs = mixed_lengths(k)
    losts, wants = [], []
    for s, r in enumerate(true_rs):
        sets = P.repair_targets(k, m, shape.r, P.cut_unit(CELL, r))
        lost, want = sets[s % len(sets)]
        losts.append(lost)
        wants.append(want)
    nbytes = cod.reconstruct_crc_rows_mixed_workspace_size(len(sb))
    buf, ws = banded(nbytes, dev)
    c = Case(cod, k, m, CELL, true_rs, losts, dev, wants=wants, expected=modes[0], pad=16, ctype=ctype)
    assert all(len(w) == shape.r for w in c.wants)
    c.mixed(workspace=ws, stripe_bytes=sb)
    runs.append((("mixed",), c))
    torch.cuda.synchronize()
    for what, c in runs:
        assert not c.dirty
        c.check((shape,) + what)
    assert bands_intact(buf, nbytes)


# ---- encode ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.ENCODE_SHAPES, ids=P.shape_id)
def test_encode_shape(dev, shape):
    """RS(k,m) for every (k, m): the rows are the m parity units."""
    k, m, full = shape.k, shape.m, shape.k * CELL
    cod, ctype = coder(k, m), CT[shape.kind]
    runs = []
    for li, r in enumerate(P.shape_lengths(k)):
        c = Enc(cod, k, m, CELL, [full] * (S_UNIFORM - 1) + [r], dev, pad=(48, 0)[li % 2], ctype=ctype)
        c.uniform()
        runs.append((("uniform", r), c))
    sb, true_rs = mixed_lengths(k)
    nbytes = cod.encode_crc_rows_mixed_workspace_size(len(sb))
    buf, ws = banded(nbytes, dev)
    c = Enc(cod, k, m, CELL, true_rs, dev, pad=16, ctype=ctype)
    c.mixed(stripe_bytes=sb, workspace=ws)
    runs.append((("mixed",), c))
    torch.cuda.synchronize()
    for what, c in runs:
        c.check((shape,) + what)
    assert bands_intact(buf, nbytes)


# ---- scrub ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.SCRUB_SHAPES, ids=P.shape_id)
def test_scrub_shape(dev, shape):
    """E extras: RS(k,E) complete in the uniform form; RS(k,4) with every
    choice of 4 - E absent parity units, and with a data unit absent in place of
    one of them, in the mixed form.  Clean, and with one byte of the short
    stripe flipped below its unit's length."""
    k, e, ctype = shape.k, shape.e, CT[shape.kind]
    full = k * CELL
    cod = coder(k, e)
    last = S_UNIFORM - 1
    runs = []
    for li, r in enumerate(P.shape_lengths(k)):
        rs = [full] * last + [r]
        lens = P.unit_lens(k, k + e, CELL, r)
        cu = P.cut_unit(CELL, r)
        hits = [(cu, lens[cu] - 1), (0, 0), (k + e - 1, min(CELL, r) - 1), (k, min(CELL, r) // 2)]
        for corrupt in ([], [(last,) + hits[li % len(hits)]]):
            b = Batch("rs", k, e, CELL, rs, dev, corrupt=corrupt, ctype=ctype)
            b.uniform(cod)
            assert int(b.want_bad.sum()) == len(corrupt) and bool(b.want_res.any()) == bool(corrupt)
            runs.append((("uniform", r, tuple(corrupt)), b))
    m = P.SHAPE_M
    n = k + m
    cod4 = coder(k, m)
    sb, true_rs = mixed_lengths(k)
    absent = P.scrub_absent_sets(k, e)
    losts = [absent[s % len(absent)] for s in range(len(sb))]
    corrupt = []
    for s in range(1, len(sb), 3):
        lens = P.unit_lens(k, n, CELL, true_rs[s])
        pres = [u for u in range(n) if u not in losts[s] and lens[u]]
        u = pres[s % len(pres)]
        corrupt.append((s, u, (977 * s) % lens[u]))
    nbytes = cod4.scrub_crc_rows_mixed_workspace_size(len(sb))
    buf, ws = banded(nbytes, dev)
    b = Batch("rs", k, m, CELL, true_rs, dev, masks=[present_mask(n, l) for l in losts], corrupt=corrupt, ctype=ctype)
    assert int(b.want_bad.sum()) == len(corrupt) == int((b.want_res[:, 1] != 0).sum())
    b.mixed(cod4, ws=ws, stripe_bytes=sb)
    runs.append((("mixed",), b))
    torch.cuda.synchronize()
    for what, b in runs:
        b.check((shape,) + what)
    assert bands_intact(buf, nbytes)


# ---- read -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.READ_SHAPES, ids=P.shape_id)
def test_read_shape(dev, shape):
    """RS(k,4), shape.r lost data units nearest the cut, without and with a
    lost parity unit; CRC32C, CRC32 and no verification."""
    k, m, full = shape.k, shape.m, shape.k * CELL
    cod = coder(k, m)
    kw = dict(verify=shape.verify is not None, ctype=CT[shape.verify or "crc32c"])
    runs = []
    for li, r in enumerate(P.shape_lengths(k)):
        rs = [full] * (S_UNIFORM - 1) + [r]
        for lost in P.read_losses(k, m, shape.r, P.cut_unit(CELL, r)):
            c = ReadCase(cod, k, m, CELL, rs, [lost] * S_UNIFORM, dev, pad=(0, 48)[li % 2], **kw)
            c.uniform()
            runs.append((("uniform", r, lost), c))
    sb, true_rs = mixed_lengths(k)
    losts = []
    for s, r in enumerate(true_rs):
        sets = P.read_losses(k, m, shape.r, P.cut_unit(CELL, r))
        losts.append(sets[s % len(sets)])
    nbytes = cod.read_crc_rows_mixed_workspace_size(len(sb))
    buf, ws = banded(nbytes, dev)
    c = ReadCase(cod, k, m, CELL, true_rs, losts, dev, pad=16, **kw)
    c.mixed(workspace=ws, stripe_bytes=sb)
    runs.append((("mixed",), c))
    torch.cuda.synchronize()
    for what, c in runs:
        assert not c.dirty
        c.check((shape,) + what)
    assert bands_intact(buf, nbytes)
