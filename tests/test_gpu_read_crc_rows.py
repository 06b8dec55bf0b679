"""Verified striped read into a file-order buffer on the GPU:
hec_read_crc_rows_device (data_len: a short last stripe) and
hec_read_crc_rows_device_mixed (one mask and one length per stripe) -- the
one-pass gf_read_rows kernel and the byte-wise gf_read_rows_bytes.  Ground truth
is the CPU oracle throughout, bit for bit, as test_gpu_reconstruct_crc_rows.py
builds it (stripes_truth, stripes_sums).  The whole-buffer-image discipline of
that file: 0xEE in every slot byte at or past len(u), in lost slots and between
cell_len and the stride; a file buffer exactly as long as the call needs, filled
with 0xA5, between two 0xC3 guard bands in the same allocation; after a call
the ENTIRE file allocation, the entire shard buffer (unchanged), the expected
sums (unchanged) and the flags must equal their images (only [0, r) of its row
is free in a flagged stripe), so a read of a byte past a unit's length, a write
at or past a stripe's end or between k * cell_len and the stride shows as well
as a wrong byte."""
import numpy as np
import pytest

import hdfs_native_ec as H
from composite_crc_cases import data_len_cases
from test_gpu_reconstruct_crc import GARBAGE, coder, present_mask, slots, stream
from test_gpu_reconstruct_crc_rows import Case as RepairCase
from test_gpu_reconstruct_crc_rows import last_short, stripes_sums, stripes_truth
from test_gpu_reconstruct_sums import short_losses

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
FILEFILL = 0xA5
GUARD = 0xC3
BAND = 256  # bytes of each guard band (a multiple of 16: the file keeps the allocation's alignment)
FLAGFILL = 0x77  # the flags buffer of a call without d_expected


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def r_values(k, cell):
    """The issue's list of r, each where it fits the shape."""
    full = k * cell
    xs = [1, 15, 16, 17, 511, 512, 513, cell - 1, cell, cell + 1, 2 * cell + 16, 2 * cell + 529, full - 1, full]
    return [r for r in dict.fromkeys(xs) if 1 <= r <= full]


def loss_sets(k, m, cell, r):
    """Nothing lost; each single data unit; the cut unit; a unit that is empty
    in the short stripe; min(4, m) data units together (those nearest the cut);
    one data unit plus one parity unit."""
    cu = (r - 1) // cell
    sets = [()] + [(u,) for u in range(k)] + [(cu,)]
    if cu + 1 < k:
        sets.append((cu + 1,))
    near = sorted(range(k), key=lambda u: (abs(u - cu), u))[:min(4, m, k)]
    sets.append(tuple(sorted(near)))
    if m >= 2:
        sets.append((cu, k))
        sets.append((0, k + 1))
    return list(dict.fromkeys(sets))


def survivors(n, k, lost):
    return [u for u in range(n) if u not in lost][:k]


class ReadCase:
    """One call's buffers and their expected images.

    rs[s] = the logical bytes of stripe s; losts[s] = the units stripe s lacks.
    corrupt = [(stripe, unit, byte)]: that slot byte of a present cell is
    flipped; corrupt_sums = [(stripe, unit, chunk)]: that expected sum instead.
    verify=False: d_expected is NULL and the flags buffer, filled with 0x77,
    must stay so.  pad widens the shard slots, base_off moves the shard buffer
    and the file off the 16-B grid, file_stride 0 = k * cell."""

    def __init__(self, cod, k, m, cell, rs, losts, dev, verify=True, corrupt=(), corrupt_sums=(), pad=0, base_off=0,
                 bpc=512, ctype=C32C, file_stride=0, seed=0):
        t, lens = stripes_truth(k, m, cell, rs, seed)
        true = stripes_sums(k, m, cell, rs, bpc, ctype, seed)
        S, n = len(rs), k + m
        self.cod, self.S, self.n, self.k, self.m, self.cell, self.bpc, self.ctype = cod, S, n, k, m, cell, bpc, ctype
        self.rs, self.lens, self.t, self.verify = list(rs), lens, t, verify
        self.losts = [tuple(l) for l in losts]
        self.file_stride = file_stride
        self.stride = file_stride or k * cell
        width = cell + pad
        host = np.full((S, n, width), GARBAGE, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if u not in self.losts[s]:
                    host[s, u, :lens[s][u]] = t[s, u, :lens[s][u]]
        for (s, u, b) in corrupt:
            assert u not in self.losts[s]
            host[s, u, b] ^= 0x40
        self.raw = torch.full((S * n * width + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = self.raw[base_off:].view(S, n, width)
        self.cells.copy_(torch.from_numpy(host).to(dev))
        self.exp_raw = self.raw.clone()
        # the file: exactly what the call needs, between the guard bands
        self.total = (S - 1) * self.stride + self.rs[-1]
        image = np.full((BAND + base_off + self.total + BAND,), GUARD, dtype=np.uint8)
        self.file_at = BAND + base_off
        image[self.file_at:self.file_at + self.total] = FILEFILL
        self.alloc = torch.from_numpy(image).to(dev)
        self.file = self.alloc[self.file_at:self.file_at + self.total]
        for s in range(S):
            row = self.file_at + s * self.stride
            image[row:row + self.rs[s]] = np.ascontiguousarray(t[s, :k]).reshape(-1)[:self.rs[s]]
        self.exp_alloc = torch.from_numpy(image).to(dev)
        self.expected = torch.from_numpy(true.copy()).to(dev)  # [S, n, nck, 4], SENT past the live chunks
        for (s, u, c) in corrupt_sums:
            assert u not in self.losts[s] and c < -(-lens[s][u] // bpc)
            self.expected[s, u, c, 3] ^= 1
        self.exp_expected = self.expected.clone()
        self.bad = torch.full((S, n), 0 if verify else FLAGFILL, dtype=torch.uint8, device=dev)
        self.exp_bad = self.bad.clone()
        self.dirty = set()
        hits = [(s, u) for (s, u, b) in corrupt if b < lens[s][u]] + [(s, u) for (s, u, _) in corrupt_sums]
        for (s, u) in hits:
            if u in survivors(n, k, self.losts[s]):
                self.dirty.add(s)
                if verify:
                    self.exp_bad[s, u] = 1

    def chk_args(self):
        return dict(file_stride=self.file_stride, expected_ptr=self.expected.data_ptr() if self.verify else None,
                    bad_ptr=self.bad.data_ptr(), bytes_per_checksum=self.bpc, checksum_type=self.ctype)

    def data_len(self):
        """The uniform form's data_len: only the last stripe may be short."""
        full = self.k * self.cell
        assert all(r == full for r in self.rs[:-1])
        return 0 if self.rs[-1] == full else (self.S - 1) * full + self.rs[-1]

    def shard_args(self, lost=None):
        ptrs, strides = slots(self.cells)
        if lost is not None:
            ptrs = [None if i in lost else p for i, p in enumerate(ptrs)]
        return ptrs, strides

    def uniform(self, strm=None):
        assert len(set(self.losts)) == 1
        ptrs, strides = self.shard_args(self.losts[0])
        self.cod.read_crc_rows_device(ptrs, strides, self.file.data_ptr(), self.cell, self.S, data_len=self.data_len(),
                                      stream=stream() if strm is None else strm, **self.chk_args())

    def mixed(self, workspace=None, stripe_bytes="rs", losts=None):
        ptrs, strides = self.shard_args()
        masks = [present_mask(self.n, l) for l in (self.losts if losts is None else losts)]
        if workspace is None:
            workspace = torch.empty(self.cod.read_crc_rows_mixed_workspace_size(self.S), dtype=torch.uint8,
                                    device=self.cells.device)
        self.workspace = workspace
        self.cod.read_crc_rows_device_mixed(ptrs, strides, self.file.data_ptr(), masks,
                                            self.rs if stripe_bytes == "rs" else stripe_bytes, self.cell, self.S,
                                            workspace.data_ptr(), workspace.numel(), stream=stream(),
                                            **self.chk_args())

    def check(self, what="", dirty=None):
        """After a synchronize: everything equals its image; in a stripe that
        read a corrupt survivor the row's [0, r) is unspecified, everything
        else still holds."""
        dirty = self.dirty if dirty is None else dirty
        assert torch.equal(self.bad, self.exp_bad), (what, "flags", self.bad.nonzero().tolist(),
                                                     self.exp_bad.nonzero().tolist())
        assert torch.equal(self.raw, self.exp_raw), (what, "the shard buffer changed")
        assert torch.equal(self.expected, self.exp_expected), (what, "the expected sums changed")
        got, want = self.alloc, self.exp_alloc
        if dirty:
            got, want = got.clone(), want.clone()
            for s in dirty:
                row = self.file_at + s * self.stride
                got[row:row + self.rs[s]] = 0
                want[row:row + self.rs[s]] = 0
        if not torch.equal(got, want):
            first = int((got != want).nonzero()[0]) - self.file_at
            raise AssertionError((what, "file", "first offset", first, "stripe", first // self.stride, "in row",
                                  first % self.stride, "rs", self.rs, "lost", self.losts[0], "total", self.total))

    def no_change(self, what=""):
        assert torch.equal(self.bad, torch.full_like(self.bad, 0 if self.verify else FLAGFILL)), what
        assert torch.equal(self.raw, self.exp_raw), what
        assert torch.equal(self.expected, self.exp_expected), what
        assert bool((self.file == FILEFILL).all()), what
        assert bool((self.alloc[:self.file_at] == GUARD).all()) and bool((self.alloc[-BAND:] == GUARD).all()), what


# ---- 1. short last stripe, fused shapes ---------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("cell", [9232, 50192])
@pytest.mark.parametrize("k,m", [(6, 3), (3, 2), (10, 4), (2, 1)])
def test_fused_shapes(dev, k, m, cell, ctype):
    """gf_read_rows, uniform form, S = 3: every r of the list, every loss set
    of loss_sets, R = 0 .. min(4, m)."""
    S = 3
    cod = coder(k, m)
    cases = []
    for r in r_values(k, cell):
        rs = [k * cell] * (S - 1) + [r]
        for lost in loss_sets(k, m, cell, r):
            assert len(lost) <= m
            c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev, pad=48, ctype=ctype)
            c.uniform()
            cases.append(c)
    torch.cuda.synchronize()
    assert len(cases) == sum(len(loss_sets(k, m, cell, r)) for r in r_values(k, cell)) >= 30
    assert any(sum(u < k for u in c.losts[0]) == min(4, m, k) for c in cases)
    for c in cases:
        assert not c.dirty
        assert c.file.data_ptr() % 16 == 0 and c.cells.data_ptr() % 16 == 0
        c.check((c.rs[-1], c.losts[0]))


# ---- 2. no loss reads no parity -----------------------------------------------------

@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (10, 4, 50192, 512), (6, 3, 1000, 100), (4, 2, 528, 512)])
def test_no_loss_reads_no_parity(dev, k, m, cell, bpc):
    """e = 0: the parity slots hold bytes and expected sums that would flag if
    they were read or verified (all units "present", or parity units lost);
    no flag, the file exact."""
    S, full = 3, k * cell
    cod = coder(k, m)
    rng = np.random.default_rng(cell + k)
    runs = []
    for r in (full, cell + 17, 1):
        rs = [full] * (S - 1) + [r]
        for lost in ((), (k,), tuple(range(k, k + m))):
            for form in ("uniform", "mixed"):
                c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev, bpc=bpc)
                junk = torch.from_numpy(rng.integers(0, 256, (S, m, c.cells.shape[2]), dtype=np.uint8)).to(dev)
                c.cells[:, k:] = junk
                c.exp_raw = c.raw.clone()
                c.expected[:, k:] ^= 0x5A
                c.exp_expected = c.expected.clone()
                c.uniform() if form == "uniform" else c.mixed()
                runs.append((c, r, lost, form))
    torch.cuda.synchronize()
    for c, r, lost, form in runs:
        assert int(c.exp_bad.sum()) == 0
        c.check((r, lost, form))


# ---- 3. the byte-wise route ---------------------------------------------------------

@pytest.mark.parametrize("shape", ["rs42", "bpc1024", "bpc100", "base1", "cell528", "cell1000", "rs65", "stride7"])
def test_bytewise_route(dev, shape):
    """The shapes the one-pass kernel does not take run gf_read_rows_bytes: same
    images.  rs65 loses five data units (two launches of rows), stride7 has a
    file_stride of k * cell_len + 7."""
    k, m, cell, kw = 6, 3, 9232, {}
    if shape == "rs42":
        k, m = 4, 2
    elif shape == "bpc1024":
        kw["bpc"] = 1024
    elif shape == "bpc100":
        kw["bpc"] = 100
    elif shape == "base1":
        kw["base_off"] = 1
    elif shape == "cell528":
        k, m, cell = 4, 2, 528
    elif shape == "cell1000":
        cell = 1000
    elif shape == "rs65":
        k, m, cell = 6, 5, 1000
    elif shape == "stride7":
        kw["file_stride"] = k * cell + 7
    S, full = 3, k * cell
    cod = coder(k, m)
    cu = max(1, k // 2)
    lengths = data_len_cases(k, cell, S) + [(S - 1) * full + r
                                            for r in (cu * cell + 1, cu * cell + 17, cu * cell + cell - 1, 77, cell)]
    cases = []
    for li, data_len in enumerate(dict.fromkeys(lengths)):
        rs = last_short(k, cell, S, data_len)
        losses = [(0, 2, 3, 4, 5), (1, 3, 6, 8, 10)] if shape == "rs65" else [()] + short_losses(k, m, cell, S, data_len)
        for ci, lost in enumerate(losses):
            if len(lost) > m:
                continue
            c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev, verify=(li + ci) % 3 != 0, pad=7,
                         ctype=(C32C, C32)[li % 2], **kw)
            c.uniform() if (li + ci) % 2 == 0 else c.mixed()
            cases.append(c)
    if shape == "base1":
        assert cases[0].cells.data_ptr() % 16 == 1 and cases[0].file.data_ptr() % 16 == 1
    torch.cuda.synchronize()
    for c in cases:
        c.check((shape, c.rs[-1], c.losts[0], c.verify))


# ---- 4. flags -----------------------------------------------------------------------

@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (10, 4, 9232, 512), (6, 3, 1000, 100)])
def test_flags(dev, k, m, cell, bpc):
    """A flipped byte below len(u) of a survivor, or a flipped expected sum:
    exactly that flag, only that row's [0, r) free.  A flipped byte at or past
    len(u), or in a present unit that is not a survivor: nothing.  After the
    flagged unit is cleared from that stripe's mask, a second mixed call makes
    the whole file exact."""
    n, S, full = k + m, 3, k * cell
    cu = max(1, k // 2)
    x = 513 if bpc == 512 else 317  # the cut unit's bytes: a short last chunk
    rs = [full] * (S - 1) + [cu * cell + x]
    lost = (0,)
    cod = coder(k, m)
    spare = survivors(n, k + 1, lost)[-1]  # present, and not among the first k
    kw = dict(bpc=bpc)
    runs = [
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(S - 1, cu, x - 1)], **kw),
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(S - 1, 1, cell // 2)], **kw),
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt_sums=[(S - 1, cu, (x - 1) // bpc)], **kw),
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(0, k, 5)], **kw),  # a parity survivor, a full stripe
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(S - 1, cu, x)], **kw),
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(S - 1, cu + 1, 0)], **kw),  # an empty unit's slot
        ReadCase(cod, k, m, cell, rs, [lost] * S, dev, corrupt=[(1, spare, 7), (S - 1, spare, 0)], **kw),
    ]
    for i, c in enumerate(runs):
        c.mixed() if i % 2 else c.uniform()
    torch.cuda.synchronize()
    for i, c in enumerate(runs):
        if i < 4:
            assert len(c.dirty) == 1 and int(c.exp_bad.sum()) == 1
        else:
            assert not c.dirty and int(c.exp_bad.sum()) == 0
        c.check(i)
    # the caller's second call: the flagged unit out of that stripe's mask
    for i, c in enumerate(runs[:4]):
        (s, u), = c.exp_bad.nonzero().tolist()
        if i == 2:
            c.expected[s, u] = torch.from_numpy(stripes_sums(k, m, cell, rs, bpc, C32C)[s, u].copy()).to(dev)
            c.exp_expected = c.expected.clone()
            again = c.losts
        else:
            again = [l + (u,) if si == s else l for si, l in enumerate(c.losts)]
        c.mixed(losts=again)
    torch.cuda.synchronize()
    for i, c in enumerate(runs[:4]):
        c.check(("second call", i), dirty=())


# ---- 5. one mask and one length per stripe ------------------------------------------

def mixed_batch(k, m, cell, S=12):
    """Lengths drawn from the r list with zeros and full ones among them, six
    distinct masks, e = 0 among them."""
    n, full = k + m, k * cell
    cycle = [0, full] + r_values(k, cell)
    rs = [cycle[(5 * s + 1) % len(cycle)] for s in range(S)]
    rs[0], rs[3], rs[7] = 0, full, 2 * cell + 529
    patterns = [(), (1,), (k - 1, k), (k + 1,), (0, 2), tuple(range(min(4, m))), (1,), (), (k,), (0, 2), (1,), (k - 1, k)]
    losts = [tuple(sorted(patterns[s % len(patterns)])) for s in range(S)]
    assert len(set(losts)) >= 5 and () in losts
    return rs, losts


@pytest.mark.parametrize("route", ["fused", "bytes"])
@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_lengths_and_patterns(dev, k, m, route):
    """12 stripes, per-stripe masks and lengths; the workspace of exactly the
    advertised size keeps its guard bands; stripe_bytes NULL is all full."""
    cell = 9232 if route == "fused" else 1000
    bpc = 512 if route == "fused" else 100
    rs, losts = mixed_batch(k, m, cell)
    S, full = len(rs), k * cell
    true_rs = [r or full for r in rs]
    cod = coder(k, m)
    nbytes = cod.read_crc_rows_mixed_workspace_size(S)
    buf = torch.full((nbytes + 512,), GUARD, dtype=torch.uint8, device=dev)
    ws = buf[256:256 + nbytes]
    assert ws.data_ptr() % 8 == 0
    a = ReadCase(cod, k, m, cell, true_rs, losts, dev, pad=16, bpc=bpc)
    a.mixed(workspace=ws, stripe_bytes=rs)
    torch.cuda.synchronize()  # the workspace is a's until the stream has passed the call
    b = ReadCase(cod, k, m, cell, true_rs, losts, dev, verify=False, bpc=bpc, ctype=C32, file_stride=full + 32)
    b.mixed(stripe_bytes=rs)
    c = ReadCase(cod, k, m, cell, [full] * S, losts, dev, bpc=bpc)
    c.mixed(stripe_bytes=None)
    d = ReadCase(cod, k, m, cell, [full] * S, losts, dev, bpc=bpc, ctype=C32)
    d.mixed(stripe_bytes=[0, full] * (S // 2))
    torch.cuda.synchronize()
    a.check("verified")
    b.check("plain, wide stride")
    c.check("stripe_bytes NULL")
    d.check("stripe_bytes 0 / full")
    assert bool((buf[:256] == GUARD).all()) and bool((buf[256 + nbytes:] == GUARD).all())


# ---- 6. no verification -------------------------------------------------------------

@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (3, 2, 50192, 512), (4, 2, 1000, 100)])
def test_no_verification(dev, k, m, cell, bpc):
    """d_expected == NULL: the same file image, the flags buffer untouched,
    also where a survivor's sums would not match."""
    S, full = 3, k * cell
    cod = coder(k, m)
    runs = []
    for r in (full, cell + 1, 2 * cell - 1 if k > 2 else cell - 1):
        rs = [full] * (S - 1) + [r]
        for lost in ((), (0,), (1, k)):
            if len(lost) > m:
                continue
            for form in ("uniform", "mixed"):
                c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev, verify=False, bpc=bpc)
                c.expected ^= 0x11  # never looked at
                c.exp_expected = c.expected.clone()
                c.uniform() if form == "uniform" else c.mixed()
                runs.append((c, r, lost, form))
    torch.cuda.synchronize()
    for c, r, lost, form in runs:
        assert bool((c.bad == FLAGFILL).all())
        c.check((r, lost, form))


# ---- 7. write -> read ---------------------------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (3, 2, 528), (4, 2, 1000)])
def test_write_then_read(dev, k, m, cell, ctype):
    """hec_encode_crc_rows_device from a file-order buffer that holds exactly
    data_len file bytes, units dropped, hec_read_crc_rows_device with the sums
    the encode wrote into a second buffer of exactly data_len bytes: equal, no
    flags.  The source allocation covers whole rows, as both calls ask of
    slots they read (a cut unit's slot may be read up to cell_len); what lies
    behind data_len in it is 0xEE.  The destination is data_len bytes between
    guard bands."""
    n, S, bpc, full = k + m, 3, 512, k * cell
    cod = coder(k, m)
    nck = -(-cell // bpc)
    rng = np.random.default_rng(cell + k + ctype)
    runs = []
    for data_len in data_len_cases(k, cell, S):
        nbytes = data_len or S * full
        rows = torch.full((S * full,), GARBAGE, dtype=torch.uint8, device=dev)
        src = rows[:nbytes]
        src.copy_(torch.from_numpy(rng.integers(0, 256, (nbytes,), dtype=np.uint8)).to(dev))
        parity = torch.full((S, m, cell), GARBAGE, dtype=torch.uint8, device=dev)
        sums = torch.full((S, n, nck, 4), 0xA5, dtype=torch.uint8, device=dev)
        dptrs = [src.data_ptr() + i * cell for i in range(k)]
        pptrs, pstrides = slots(parity)
        cod.encode_crc_rows_device(dptrs, [full] * k, pptrs, pstrides, cell, S, sums.data_ptr(), data_len=data_len,
                                   bytes_per_checksum=bpc, checksum_type=ctype, stream=stream())
        for lost in [()] + short_losses(k, m, cell, S, data_len):
            if len(lost) > m:
                continue
            ptrs = [None if i in lost else p for i, p in enumerate(dptrs + pptrs)]
            alloc = torch.full((BAND + nbytes + BAND,), GUARD, dtype=torch.uint8, device=dev)
            dst = alloc[BAND:BAND + nbytes]
            dst.fill_(FILEFILL)
            bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
            cod.read_crc_rows_device(ptrs, [full] * k + pstrides, dst.data_ptr(), cell, S, data_len=data_len,
                                     expected_ptr=sums.data_ptr(), bad_ptr=bad.data_ptr(), bytes_per_checksum=bpc,
                                     checksum_type=ctype, stream=stream())
            runs.append((data_len, lost, src, alloc, dst, bad))
    torch.cuda.synchronize()
    for data_len, lost, src, alloc, dst, bad in runs:
        assert not bool(bad.any()), (data_len, lost, bad.nonzero().tolist())
        assert torch.equal(dst, src), (data_len, lost)
        assert bool((alloc[:BAND] == GUARD).all()) and bool((alloc[-BAND:] == GUARD).all()), (data_len, lost)


# ---- 8. agreement with the repair ---------------------------------------------------

@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (10, 4, 9232, 512), (6, 3, 1000, 100)])
def test_agrees_with_the_repair(dev, k, m, cell, bpc):
    """The lost data units' [0, len(t)) equal what
    hec_reconstruct_crc_rows_device_mixed writes on the same batch."""
    rs, losts = mixed_batch(k, m, cell)
    full = k * cell
    true_rs = [r or full for r in rs]
    cod = coder(k, m)
    rep = RepairCase(cod, k, m, cell, true_rs, losts, dev, expected="sep", separate=True, bpc=bpc)
    rep.mixed(stripe_bytes=rs)
    c = ReadCase(cod, k, m, cell, true_rs, losts, dev, bpc=bpc)
    c.mixed(stripe_bytes=rs)
    torch.cuda.synchronize()
    c.check()
    compared = 0
    for s, lost in enumerate(losts):
        for t_ in lost:
            if t_ < k and c.lens[s][t_]:
                at = s * c.stride + t_ * cell
                assert torch.equal(c.file[at:at + c.lens[s][t_]], rep.out[s, t_, :c.lens[s][t_]]), (s, t_)
                compared += 1
    assert compared >= 4


# ---- 9. graph -----------------------------------------------------------------------

def test_graph_capture_replay(dev):
    """The uniform form with a short last stripe captured on a side stream and
    replayed three times over changed inputs."""
    k, m, S, cell = 6, 3, 3, 9232
    rs = [k * cell] * (S - 1) + [3 * cell + 513]
    cod = coder(k, m)
    lost = (3, k)
    c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev)
    others = [ReadCase(cod, k, m, cell, rs, [lost] * S, dev, seed=seed,
                       corrupt=[(S - 1, 1, 100)] if seed == 2 else ()) for seed in (1, 2, 3)]
    c.uniform()  # eager once, then captured
    torch.cuda.synchronize()
    c.check("eager")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.uniform()
    for rep, o in enumerate(others):
        c.raw.copy_(o.raw)
        c.expected.copy_(o.expected)
        c.alloc.copy_(o.alloc)
        c.bad.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.exp_raw, c.exp_expected, c.exp_alloc, c.exp_bad = o.exp_raw, o.exp_expected, o.exp_alloc, o.exp_bad
        c.check(("replay", rep), dirty=o.dirty)
        assert int(c.bad.sum()) == (1 if rep == 1 else 0)


# ---- 10. tensor helper --------------------------------------------------------------

def test_tensor_helper(dev):
    k, m, cell = 6, 3, 9232
    n, full = k + m, k * cell
    cod = coder(k, m)
    rs, losts = mixed_batch(k, m, cell)
    a = ReadCase(cod, k, m, cell, [r or full for r in rs], losts, dev)
    ws = H.read_crc_rows_batch(cod, a.cells, [present_mask(n, l) for l in losts], a.expected, a.file, stripe_bytes=rs,
                               bad=a.bad)
    assert ws.numel() >= cod.read_crc_rows_mixed_workspace_size(len(rs))
    S = 3
    urs = [full] * (S - 1) + [cell + 17]
    b = ReadCase(cod, k, m, cell, urs, [(1,)] * S, dev)
    assert H.read_crc_rows_batch(cod, b.cells, [present_mask(n, (1,))] * S, b.expected, b.file, data_len=b.data_len(),
                                 bad=b.bad) is None
    d = ReadCase(cod, k, m, cell, urs, [(1,), (), (0, k)], dev, verify=False)
    H.read_crc_rows_batch(cod, d.cells, [present_mask(n, l) for l in d.losts], None, d.file, data_len=d.data_len())
    with pytest.raises(ValueError):
        H.read_crc_rows_batch(cod, d.cells, [present_mask(n, l) for l in d.losts], None, d.file, data_len=5,
                              stripe_bytes=urs)
    torch.cuda.synchronize()
    a.check("mixed")
    b.check("uniform")
    d.check("data_len with several masks")


# ---- 11. argument errors on the device, nothing queued ------------------------------

def test_argument_errors_write_nothing(dev):
    k, m, n, S, cell = 6, 3, 9, 4, 9232
    cod = coder(k, m)
    full = k * cell
    rs = [full] * (S - 1) + [cell + 5]
    lost = (1, 7)
    c = ReadCase(cod, k, m, cell, rs, [lost] * S, dev)
    ptrs, strides = c.shard_args()
    shards = [None if i in lost else p for i, p in enumerate(ptrs)]
    masks = [present_mask(n, lost)] * S
    ws = torch.empty(cod.read_crc_rows_mixed_workspace_size(S) + 16, dtype=torch.uint8, device=dev)
    fp, wp, wn = c.file.data_ptr(), ws.data_ptr(), ws.numel()
    ep, bp = c.expected.data_ptr(), c.bad.data_ptr()

    def uniform(shards_=shards, strides_=strides, file_=fp, S_=S, data_len=c.data_len(), **kw):
        kw = {**dict(expected_ptr=ep, bad_ptr=bp), **kw}
        cod.read_crc_rows_device(shards_, strides_, file_, cell, S_, data_len=data_len, stream=stream(), **kw)

    def mixed(ptrs_=ptrs, strides_=strides, file_=fp, masks_=masks, lens=rs, S_=S, w=wp, wbytes=wn, **kw):
        kw = {**dict(expected_ptr=ep, bad_ptr=bp), **kw}
        cod.read_crc_rows_device_mixed(ptrs_, strides_, file_, masks_, lens, cell, S_, w, wbytes, stream=stream(), **kw)

    def both(**kw):
        with pytest.raises(ValueError):
            uniform(**kw)
        with pytest.raises(ValueError):
            mixed(**kw)

    both(checksum_type=H.CHECKSUM_NULL)
    both(checksum_type=7)
    both(bytes_per_checksum=0)
    both(file_=None)
    both(strides_=None)
    both(expected_ptr=ep + 2)
    both(expected_ptr=ep, bad_ptr=None)
    for stride in (16, full - 16, full - 1):
        both(file_stride=stride)
    with pytest.raises(ValueError):
        uniform(shards_=None)
    with pytest.raises(ValueError):
        mixed(ptrs_=None)
    with pytest.raises(ValueError):
        mixed(masks_=None)
    for S_, data_len in ((S, (S - 1) * full), (S, 1), (S, S * full + 1), (0, 5)):
        with pytest.raises(ValueError):
            uniform(S_=S_, data_len=data_len)
    with pytest.raises(ValueError):
        mixed(lens=[full + 1] + rs[1:])
    # a survivor without storage (mixed form)
    with pytest.raises(ValueError):
        mixed(ptrs_=[None if i == 0 else p for i, p in enumerate(ptrs)])
    # fewer than k units present
    with pytest.raises(H.ErasureCodingError):
        uniform(shards_=[None] * 4 + ptrs[4:])
    with pytest.raises(H.ErasureCodingError):
        mixed(masks_=masks[:-1] + [present_mask(n, (1, 2, 7, 8))])
    # a workspace that is too small, NULL or misaligned
    for p, nbytes in ((wp, cod.read_crc_rows_mixed_workspace_size(S) - 8), (wp, 8), (None, wn), (wp + 4, wn - 4)):
        with pytest.raises(ValueError):
            mixed(w=p, wbytes=nbytes)
    torch.cuda.synchronize()
    c.no_change("errors")
    # no stripes: OK, and still nothing written
    uniform(S_=0, data_len=0)
    mixed(masks_=[], lens=[], S_=0)
    torch.cuda.synchronize()
    c.no_change("no stripes")
    # and the same arguments without a fault in them do the read
    uniform()
    torch.cuda.synchronize()
    c.check("valid")
