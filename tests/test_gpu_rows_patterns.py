"""Every loss pattern at every cut through the mixed forms of the short-stripe
repair, read and scrub on the GPU.

rows_shape_cases.batch gives one batch per (code, cut unit): every set of at
most m lost units of RS(3,2), RS(6,3) and RS(10,4), each at lengths r = u * c + x
with x over X(c).  The pattern decides which unit sits in which slot of the
kernel (the survivors are the first k present units), the cut decides which of
them have ended, so together they decide which two slots share a checksum round
at different lengths, whether slot 0 is unit 0 and whether an ended unit's loads
go to a parity unit.  One mask and one length per stripe: a batch is one call.

Ground truth is the CPU oracle as test_gpu_reconstruct_crc_rows.py builds it
(stripes_truth, stripes_sums), and for the scrub the host routine with
degraded_scrub_ref as test_gpu_scrub_crc_rows.Batch computes it.  The images are
those of Case, ReadCase and Batch: 0xEE past every unit's length and in lost
slots, sentinel-filled outputs, sums and flags, the file between guard bands,
every buffer compared whole, inputs included.  The workspace is exactly as large
as advertised and lies between two guard bands.

Repair and read run on clean survivors: every image exact, no flag.  A clean
scrub cannot tell whether a unit was read at all, so in every second stripe one
byte below the length of one present unit is flipped (rows_shape_cases.
scrub_flips), the unit and the position rotating over the stripe index.

A batch's truth is computed once, shared by its three calls and dropped before
the next batch."""
import pytest

import hdfs_native_ec as H
import rows_shape_cases as P
from test_gpu_reconstruct_crc import coder, present_mask
from test_gpu_reconstruct_crc_rows import Case, forget_truth, stripes_sums, stripes_truth
from test_gpu_read_crc_rows import ReadCase
from test_gpu_scrub_crc_rows import Batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xC3
BAND = 256
BATCHES = P.all_batches()
CALLS = ("repair", "read", "scrub")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_current = {}


def shared_batch(index):
    """The batch and its checksum kind (CRC32C and CRC32 by turns); the truth
    of the batch before it is dropped."""
    if _current.get("index") != index:
        old = _current.get("batch")
        if old is not None:
            forget_truth(old.k, old.m, old.cell, old.rs)
        k, m, cut = BATCHES[index]
        b = P.batch(k, m, cut)
        _current.update(index=index, batch=b)
        stripes_truth(k, m, b.cell, b.rs)
    return _current["batch"], (H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32)[index % 2]


def banded(nbytes, dev):
    buf = torch.full((nbytes + 2 * BAND,), GUARD, dtype=torch.uint8, device=dev)
    ws = buf[BAND:BAND + nbytes]
    assert ws.data_ptr() % 8 == 0
    return buf, ws


def bands_intact(buf, nbytes):
    return bool((buf[:BAND] == GUARD).all()) and bool((buf[BAND + nbytes:] == GUARD).all())


@pytest.mark.parametrize("index,call", [(i, c) for i in range(len(BATCHES)) for c in CALLS],
                         ids=["rs%d_%d-cut%s-%s" % (BATCHES[i] + (c,)) for i in range(len(BATCHES)) for c in CALLS])
def test_every_pattern_at_every_cut(dev, index, call):
    b, ctype = shared_batch(index)
    k, m, cell, S = b.k, b.m, b.cell, len(b.rs)
    cod = coder(k, m)
    if call == "repair":
        # want NULL, d_expected present, in place
        c = Case(cod, k, m, cell, b.rs, b.losts, dev, expected="sep", ctype=ctype)
        nbytes = cod.reconstruct_crc_rows_mixed_workspace_size(S)
        buf, ws = banded(nbytes, dev)
        c.mixed(workspace=ws)
        torch.cuda.synchronize()
        assert not c.dirty and not bool(c.exp_bad.any())
        c.check((k, m, b.cut_units, "repair"))
    elif call == "read":
        c = ReadCase(cod, k, m, cell, b.rs, b.losts, dev, ctype=ctype)
        assert c.verify and c.file_stride == 0
        nbytes = cod.read_crc_rows_mixed_workspace_size(S)
        buf, ws = banded(nbytes, dev)
        c.mixed(workspace=ws)
        torch.cuda.synchronize()
        assert not c.dirty and not bool(c.exp_bad.any())
        c.check((k, m, b.cut_units, "read"))
    else:
        flips = P.scrub_flips(b)
        c = Batch("rs", k, m, cell, b.rs, dev, masks=[present_mask(k + m, l) for l in b.losts], corrupt=flips,
                  ctype=ctype)
        nbytes = cod.scrub_crc_rows_mixed_workspace_size(S)
        buf, ws = banded(nbytes, dev)
        c.mixed(cod, ws=ws)
        torch.cuda.synchronize()
        # every flip is below its unit's length: each sets exactly its flag, and
        # where the stripe has an extra its result word is not clean
        assert int(c.want_bad.sum()) == len(flips) == S // 2
        assert all(c.want_bad[s, u] for s, u, _ in flips)
        with_extra = [s for s, _, _ in flips if len(b.losts[s]) < m]
        assert with_extra and all(c.want_res[s, 1] for s in with_extra)
        assert not c.want_res[0::2].any()
        c.check((k, m, b.cut_units, "scrub"))
    assert bands_intact(buf, nbytes), (call, "workspace guard bands")
    if (index, call) == (len(BATCHES) - 1, CALLS[-1]):
        forget_truth(k, m, cell, b.rs)
        _current.clear()
