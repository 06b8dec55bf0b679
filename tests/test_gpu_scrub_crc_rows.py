"""Verified scrub of short stripes on the GPU: hec_scrub_crc_rows_device
(data_len: a short last stripe) and hec_scrub_crc_rows_device_mixed (one length
per stripe) -- the one-pass gf_scrub_crc_rows kernel and the byte-wise
gf_scrub_rows_bytes.

Ground truth is never the code under test.  Results: hec_scrub_degraded (the
host routine) on zero-padded host copies of the uploaded slots at shard_len =
n0, cross-checked on the dirty stripes with tests/degraded_scrub_ref.py.
Flags: the oracle's CRCs of each present unit's uploaded bytes below len(u)
against the uploaded expected words.  Whole-buffer images: present slots hold
0xEE from len(u) to the stride, lost slots are all 0xEE, the expected sums
hold the sentinel past each unit's live chunks, flags are zeroed and results
pre-filled with -1; after a call the cells and the expected sums must be
byte-identical to what was uploaded and the results and flags must equal their
full expected images."""
import numpy as np
import pytest

import degraded_scrub_ref as R
import ec_oracle as O
import hdfs_native_ec as H
from composite_crc_cases import oracle_crc
from test_gpu_reconstruct_crc import GARBAGE, SENT, chunk_sums, present_mask, stream
from test_gpu_reconstruct_crc_rows import Case, stripes_sums, stripes_truth, unit_lens
from test_gpu_reconstruct_sums import be32, clib
from test_gpu_scrub import as_u64, coder, prefilled

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
PAD = 16  # bytes between cell_len and the stride
GUARD = 0xC3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_other = {}


def truth(codec, k, m, cell, rs, bpc, ctype):
    """(cells [S, n, cell], lens [S][n], sums [S, n, nck, 4]) of a batch whose
    stripe s holds rs[s] bytes, computed once and read-only: the shared RS
    truth of test_gpu_reconstruct_crc_rows, or the same construction over
    another codec's matrix."""
    if codec == "rs":
        t, lens = stripes_truth(k, m, cell, rs)
        return t, lens, stripes_sums(k, m, cell, rs, bpc, ctype)
    key = (codec, k, m, cell, tuple(rs), bpc, ctype)
    if key not in _other:
        S, n = len(rs), k + m
        rng = np.random.default_rng(31 * k + cell + sum(rs))
        data = rng.integers(0, 256, size=(S, k * cell), dtype=np.uint8)
        for s, r in enumerate(rs):
            data[s, r:] = 0
        t = np.zeros((S, n, cell), dtype=np.uint8)
        t[:, :k] = data.reshape(S, k, cell)
        par = O.matmul_shards(O.codec_matrix(codec, k, m)[k:],
                              [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)])
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        lens = [unit_lens(k, n, cell, r) for r in rs]
        sums = np.full((S, n, -(-cell // bpc), 4), SENT, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if lens[s][u]:
                    live = chunk_sums(t[s, u, :lens[s][u]], bpc, ctype)
                    sums[s, u, :live.shape[0]] = live
        t.setflags(write=False)
        sums.setflags(write=False)
        _other[key] = (t, lens, sums)
    return _other[key]


def forget(min_bytes):
    """Drops the cached batches of at least min_bytes of cells."""
    for key in [key for key, v in _other.items() if v[0].nbytes >= min_bytes]:
        del _other[key]


class Batch:
    """One call's buffers and the expected images.

    rs[s] = the logical bytes of stripe s (k * cell: full); masks[s] = the
    present units (None: all).  corrupt = [(stripe, unit, byte)]: that slot
    byte is flipped after the upload image is made, whether it lies below the
    unit's length or not; silent = the same, and the unit's live expected sums
    are then the oracle's of its flipped bytes (visible to the parity check
    only); corrupt_sums = [(stripe, unit, word)]: that expected word, live or
    not."""

    def __init__(self, codec, k, m, cell, rs, dev, masks=None, corrupt=(), corrupt_sums=(), bpc=512, ctype=C32C,
                 base_off=0, silent=()):
        t, lens, sums = truth(codec, k, m, cell, rs, bpc, ctype)
        S, n = len(rs), k + m
        self.codec, self.k, self.m, self.n, self.S, self.cell, self.bpc, self.ctype = codec, k, m, n, S, cell, bpc, ctype
        self.rs, self.lens = [int(r) for r in rs], lens
        self.masks = [(1 << n) - 1] * S if masks is None else [int(x) for x in masks]
        img = np.full((S, n, cell + PAD), GARBAGE, dtype=np.uint8)
        simg = np.full(sums.shape, SENT, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if (self.masks[s] >> u) & 1:
                    img[s, u, :lens[s][u]] = t[s, u, :lens[s][u]]
                    simg[s, u] = sums[s, u]
        for (s, u, b) in list(corrupt) + list(silent):
            img[s, u, b] ^= 0x40
        for (s, u, _) in silent:
            live = chunk_sums(img[s, u, :lens[s][u]], bpc, ctype)
            simg[s, u, :live.shape[0]] = live
        for (s, u, c) in corrupt_sums:
            simg[s, u, c, 3] ^= 1
        self.h_cells, self.h_sums = img, simg
        flat = torch.full((img.size + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = flat[base_off:].view(S, n, cell + PAD)
        self.cells.copy_(torch.from_numpy(img).to(dev))
        self.exp = torch.from_numpy(simg).to(dev)
        self.res = prefilled(S, dev)
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        # flags: the oracle's sums of every present unit's own uploaded bytes
        self.want_bad = np.zeros((S, n), dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                ln = lens[s][u]
                if (self.masks[s] >> u) & 1 and ln:
                    live = chunk_sums(img[s, u, :ln], bpc, ctype)
                    self.want_bad[s, u] = int((live != simg[s, u, :live.shape[0]]).any())
        # results: the host routine over zero-padded copies at shard_len = n0
        host = H.Coder(k, m, H.HEC_DEVICE_HOST, codec=codec)
        self.want_res = np.zeros((S, 2), dtype=np.uint64)
        for s in range(S):
            n0 = min(cell, self.rs[s])
            units = []
            for u in range(n):
                if not (self.masks[s] >> u) & 1:
                    units.append(None)
                    continue
                x = np.zeros(n0, dtype=np.uint8)
                x[:lens[s][u]] = img[s, u, :lens[s][u]]
                units.append(x)
            ruled, nbad = host.scrub_degraded(units)
            self.want_res[s] = (ruled, nbad)
            if nbad:  # the dirty stripes once more, by rebuild and compare
                ref = R.ref_scrub(codec, k, m, units, self.masks[s])
                assert (int(ref[0]), int(ref[1])) == (int(ruled), int(nbad)), (s, ref, ruled, nbad)
        host.close()

    def slots(self):
        width = self.cell + PAD
        return [self.cells.data_ptr() + i * width for i in range(self.n)], [self.n * width] * self.n

    def data_len(self):
        full = self.k * self.cell
        assert all(r == full for r in self.rs[:-1])
        return 0 if self.rs[-1] == full else (self.S - 1) * full + self.rs[-1]

    def uniform(self, cod, st=None, data_len=None):
        ptrs, strides = self.slots()
        cod.scrub_crc_rows_device(ptrs, strides, self.cell, self.S, self.exp.data_ptr(), self.bad.data_ptr(),
                                  self.res.data_ptr(), data_len=self.data_len() if data_len is None else data_len,
                                  bytes_per_checksum=self.bpc, checksum_type=self.ctype,
                                  stream=stream() if st is None else st)

    def mixed(self, cod, ws=None, st=None, stripe_bytes="rs"):
        ptrs, strides = self.slots()
        if ws is None:
            ws = torch.full((max(cod.scrub_crc_rows_mixed_workspace_size(self.S), 1),), SENT, dtype=torch.uint8,
                            device=self.cells.device)
        self.ws = ws
        cod.scrub_crc_rows_device_mixed(ptrs, strides, self.masks, self.rs if stripe_bytes == "rs" else stripe_bytes,
                                        self.cell, self.S, self.exp.data_ptr(), self.bad.data_ptr(),
                                        self.res.data_ptr(), ws.data_ptr(), ws.numel(), bytes_per_checksum=self.bpc,
                                        checksum_type=self.ctype, stream=stream() if st is None else st)

    def reset_outputs(self):
        self.res.fill_(-1)
        self.bad.zero_()

    def check(self, what=""):
        """After a synchronize."""
        got_res = as_u64(self.res, self.S)
        got_bad = self.bad.cpu().numpy()
        assert np.array_equal(got_res, self.want_res), (what, "results", got_res.tolist(), self.want_res.tolist())
        assert np.array_equal(got_bad, self.want_bad), (what, "flags", np.argwhere(got_bad).tolist(),
                                                        np.argwhere(self.want_bad).tolist())
        assert np.array_equal(self.cells.cpu().numpy(), self.h_cells), (what, "cells were written")
        assert np.array_equal(self.exp.cpu().numpy(), self.h_sums), (what, "expected sums were written")

    def unchanged(self, what=""):
        assert bool((self.res == -1).all()), what
        assert not bool(self.bad.any()), what
        assert np.array_equal(self.cells.cpu().numpy(), self.h_cells), what
        assert np.array_equal(self.exp.cpu().numpy(), self.h_sums), what


def short_rs(k, cell, e):
    """r of the short stripe: the issue's list.  The cut unit is unit k/2; a
    wave-tile is 8 KiB where e == 1 and k <= 6, else 4 KiB."""
    cu = max(1, k // 2) if k > 1 else 0
    wave = 8192 if (e == 1 and k <= 6) else 4096
    rs = [1, 15, 16, 17, 511, 512, 513, cell - 1, cell, cell + 1, cell + 17, cu * cell + 513, k * cell - 1]
    rs += [cu * cell + w * wave + 1234 for w in range(4) if w * wave + 1234 < cell]
    return sorted(set(r for r in rs if 1 <= r < k * cell))


# ---- 1. clean short last stripe, fused shapes ----------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("cell", [9232, 50192])
@pytest.mark.parametrize("k,m", [(6, 3), (3, 2), (10, 4), (2, 1)])
def test_clean_short_last_stripe_fused_shapes(dev, k, m, cell, ctype):
    S, full = 3, k * cell
    cod = coder(k, m)
    runs = []
    for r in short_rs(k, cell, m):
        b = Batch("rs", k, m, cell, [full] * (S - 1) + [r], dev, ctype=ctype)
        b.uniform(cod)
        runs.append((r, b))
    torch.cuda.synchronize()
    for r, b in runs:
        assert not b.want_res.any() and not b.want_bad.any(), r
        b.check(("r", r))


# ---- 2. corruption in the short stripe -------------------------------------------------

def corruption_cases(k, m, cell, bpc):
    """(r, corrupt, corrupt_sums) per run; the short stripe is stripe 2."""
    n, cu = k + m, max(1, k // 2)
    s = 2
    out = []
    for r in (cu * cell + 4096 + 1234 if cell > 6000 else cu * cell + 513, cell + 17, 777):
        lens = unit_lens(k, n, cell, r)
        n0 = min(cell, r)
        cut = max(u for u in range(k) if lens[u])
        out.append((r, [(s, 0, 0)], []))
        out.append((r, [(s, cut, lens[cut] - 1)], []))
        if n0 > 4096:
            out.append((r, [(s, 0, 4096)], []))  # the first byte of a later wave-tile
        out.append((r, [(s, k + m - 1, n0 - 1)], []))
        # what must change nothing, or the flag only
        if lens[cut] < cell:
            out.append((r, [(s, cut, lens[cut])], []))  # a slot byte at the unit's length
            out.append((r, [(s, cut, cell - 1)], []))
        if n0 < cell:
            out.append((r, [(s, k, n0)], []))  # a parity byte at n0
        out.append((r, [], [(s, 0, 0)]))  # a live expected sum
        live = -(-lens[cut] // bpc)
        if live < -(-cell // bpc):
            out.append((r, [], [(s, cut, live)]))  # a sums word past the live chunks
        empty = [u for u in range(k) if lens[u] == 0]
        if empty:
            out.append((r, [(s, empty[0], 0)], [(s, empty[0], 0)]))  # anything of a length-0 unit
    return out


@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (10, 4, 9232, 512), (6, 3, 1000, 100)])
def test_corruption_in_the_short_stripe(dev, k, m, cell, bpc):
    S, full, n = 3, k * cell, k + m
    cod = coder(k, m)
    runs = []
    for (r, corrupt, corrupt_sums) in corruption_cases(k, m, cell, bpc):
        b = Batch("rs", k, m, cell, [full] * (S - 1) + [r], dev, corrupt=corrupt, corrupt_sums=corrupt_sums, bpc=bpc)
        b.uniform(cod)
        runs.append((r, corrupt, corrupt_sums, b))
    torch.cuda.synchronize()
    seen_located = 0
    for r, corrupt, corrupt_sums, b in runs:
        what = (r, corrupt, corrupt_sums)
        b.check(what)
        lens = b.lens[2]
        hit = [(s, u) for (s, u, byte) in corrupt if byte < lens[u]]
        sum_hit = [(s, u) for (s, u, c) in corrupt_sums if c < -(-lens[u] // bpc)]
        # the images above are the check; this states what they must have been
        assert b.want_bad.sum() == len(hit) + len(sum_hit), what
        if hit:
            (s, u), = hit
            assert b.want_bad[s, u] == 1, what
            verdict, unit = H.scrub_verdict(int(b.want_res[s, 0]), int(b.want_res[s, 1]), n)
            assert (verdict, unit) == (H.HEC_SCRUB_LOCATED, u), what
            seen_located += 1
        else:
            assert not b.want_res.any(), what
    assert seen_located >= 9


# ---- 3. mixed lengths and masks ------------------------------------------------------------

def mixed_batch(k, m, cell, S=24):
    n, full, cu = k + m, k * cell, max(1, k // 2)
    pool = [0, full, 1, 777, cell, cell + 17, cu * cell + 513, full - 1]
    rng = np.random.default_rng(100 * k + cell)
    rs = [pool[(s * 3 + s // 8) % len(pool)] for s in range(S)]
    losts = [(), (0,), (k + m - 1,), (cu,), (k,)]
    losts += [(u,) for u in range(n)]
    losts.append(tuple(range(1, 1 + m)))  # m lost: e == 0, sums still verified
    losts.append(tuple(range(k - 1, k + m)))  # more than m lost
    losts.append(tuple(range(0, m)))
    while len(losts) < S:
        losts.append((int(rng.integers(0, n)),))
    losts = losts[:S]
    masks = [present_mask(n, l) for l in losts]
    lens = [unit_lens(k, n, cell, r or full) for r in rs]
    corrupt, corrupt_sums = [], []
    for s in (1, 6, 11, 17):
        pres = [u for u in range(n) if u not in losts[s] and lens[s][u]]
        u = pres[s % len(pres)]
        corrupt.append((s, u, lens[s][u] - 1))
    for s in (3, 9):
        pres = [u for u in range(n) if u not in losts[s] and lens[s][u]]
        corrupt_sums.append((s, pres[-1], 0))
    for s in (4, 12):  # garbage past a unit's length: nothing
        pres = [u for u in range(n) if u not in losts[s] and lens[s][u] < cell]
        if pres:
            corrupt.append((s, pres[0], lens[s][pres[0]]))
    return rs, masks, corrupt, corrupt_sums


@pytest.mark.parametrize("cell,bpc", [(9232, 512), (1000, 512)])
@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_lengths_and_masks(dev, k, m, cell, bpc):
    cod = coder(k, m)
    rs, masks, corrupt, corrupt_sums = mixed_batch(k, m, cell)
    full = k * cell
    b = Batch("rs", k, m, cell, [r or full for r in rs], dev, masks=masks, corrupt=corrupt, corrupt_sums=corrupt_sums,
              bpc=bpc)
    b.mixed(cod, stripe_bytes=rs)
    torch.cuda.synchronize()
    assert b.want_res[:, 1].any() and b.want_bad.any()
    b.check("first run")
    # again, with a workspace of exactly the advertised size between two guard bands
    need = cod.scrub_crc_rows_mixed_workspace_size(b.S)
    assert need >= cod.scrub_crc_mixed_workspace_size(b.S)
    band = 256
    buf = torch.full((need + 2 * band,), GUARD, dtype=torch.uint8, device=dev)
    b.reset_outputs()
    b.mixed(cod, ws=buf[band:band + need], stripe_bytes=rs)
    torch.cuda.synchronize()
    b.check("banded run")
    assert bool((buf[:band] == GUARD).all()) and bool((buf[band + need:] == GUARD).all())


# ---- 4. composed / byte-wise shapes, both forms ----------------------------------------------

SHAPES = {
    "rs42": dict(codec="rs", k=4, m=2, cell=1008),
    "rs65": dict(codec="rs", k=6, m=5, cell=1008),  # e = 5
    "xor51": dict(codec="xor", k=5, m=1, cell=1008),
    "bpc1024": dict(codec="rs", k=6, m=3, cell=2064, bpc=1024),
    "bpc100": dict(codec="rs", k=6, m=3, cell=1008, bpc=100),
    "base8": dict(codec="rs", k=6, m=3, cell=1008, base_off=8),
    "cell528": dict(codec="rs", k=6, m=3, cell=528),
    "cell37": dict(codec="rs", k=3, m=2, cell=37, bpc=16),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_bytewise_shapes(dev, shape):
    p = dict(SHAPES[shape])
    codec, k, m, cell = p.pop("codec"), p.pop("k"), p.pop("m"), p.pop("cell")
    n, full, cu = k + m, k * cell, max(1, k // 2)
    cod = coder(k, m, codec)
    runs = []
    for r in (1, cell - 1, cell, cell + 1, cu * cell + min(513, cell - 1), full - 1):
        lens = unit_lens(k, n, cell, r)
        cut = max(u for u in range(k) if lens[u])
        for corrupt in ([], [(2, cut, lens[cut] - 1)], [(2, n - 1, 0)]):
            b = Batch(codec, k, m, cell, [full, full, r], dev, corrupt=corrupt, **p)
            b.uniform(cod)
            runs.append((r, corrupt, "uniform", b))
        # mixed: every stripe short, one unit lost per stripe (the last stripe: m lost)
        rs = [r, max(1, r // 2), min(full - 1, r + 5), r]
        losts = [(0,), (n - 1,), (), tuple(range(k, n))]
        b = Batch(codec, k, m, cell, rs, dev, masks=[present_mask(n, l) for l in losts], corrupt=[(2, 0, 0)], **p)
        b.mixed(cod)
        runs.append((r, "mixed", "", b))
    torch.cuda.synchronize()
    for r, what, form, b in runs:
        b.check((shape, r, what, form))


# ---- 5. full stripes identical to hec_scrub_crc_device[_mixed] ---------------------------------

@pytest.mark.parametrize("cell", [9232, 1000])
def test_full_stripes_identical(dev, cell):
    k, m, S = 6, 3, 8
    n, full = k + m, k * cell
    cod = coder(k, m)
    corrupt = [(1, 2, 5), (4, k + 1, cell - 1), (6, 0, 4097 if cell > 5000 else 600)]
    corrupt_sums = [(2, 3, 0)]
    losts = [(), (0,), (k,), (1, 2, 3), (), (n - 1,), (4,), (0, 1, 2, 3)]
    masks = [present_mask(n, l) for l in losts]
    ub = Batch("rs", k, m, cell, [full] * S, dev, corrupt=corrupt, corrupt_sums=corrupt_sums)
    mb = Batch("rs", k, m, cell, [full] * S, dev, masks=masks, corrupt=[c for c in corrupt if c[1] not in losts[c[0]]])
    ptrs, strides = ub.slots()
    ref_res, ref_bad = prefilled(S, dev), torch.zeros((S, n), dtype=torch.uint8, device=dev)
    cod.scrub_crc_device(ptrs, strides, cell, S, ub.exp.data_ptr(), ref_bad.data_ptr(), ref_res.data_ptr(),
                         stream=stream())
    for data_len in (0, S * full):
        ub.reset_outputs()
        ub.uniform(cod, data_len=data_len)
        torch.cuda.synchronize()
        ub.check(("uniform", data_len))
        assert torch.equal(ub.res, ref_res) and torch.equal(ub.bad, ref_bad), data_len
    ptrs, strides = mb.slots()
    ws = torch.empty(cod.scrub_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    ref_res, ref_bad = prefilled(S, dev), torch.zeros((S, n), dtype=torch.uint8, device=dev)
    cod.scrub_crc_device_mixed(ptrs, strides, masks, cell, S, mb.exp.data_ptr(), ref_bad.data_ptr(),
                               ref_res.data_ptr(), ws.data_ptr(), ws.numel(), stream=stream())
    for lens in (None, [0] * S, [full] * S, [0, full] * (S // 2)):
        mb.reset_outputs()
        mb.mixed(cod, stripe_bytes=lens)
        torch.cuda.synchronize()
        mb.check(("mixed", lens))
        assert torch.equal(mb.res, ref_res) and torch.equal(mb.bad, ref_bad), lens


# ---- 6. the repair loop on a short group ---------------------------------------------------------

@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (10, 4, 9232), (4, 2, 1000)])
def test_repair_then_scrub_then_composite(dev, k, m, cell):
    """reconstruct_crc_rows_device in place with d_expected == d_sums and no
    zero padding, scrub_crc_rows_device against that sums array, the composite
    fold with the same data_len; then one rebuilt byte flipped."""
    n, S, bpc = k + m, 4, 512
    cod = coder(k, m)
    full = k * cell
    runs = []
    for r in (1, 777, cell, cell + 17, max(1, k // 2) * cell + 513, full - 1):
        rs = [full] * (S - 1) + [r]
        for lost in ((0,), (max(1, k // 2), k), (k - 1, n - 1)):
            if len(lost) > m:
                continue
            c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected="same")
            c.uniform()
            data_len = c.data_len()
            ptrs, strides = c.ptr_args()[:2]
            res, bad = prefilled(S, dev), torch.zeros((S, n), dtype=torch.uint8, device=dev)
            cod.scrub_crc_rows_device(ptrs, strides, cell, S, c.sums.data_ptr(), bad.data_ptr(), res.data_ptr(),
                                      data_len=data_len, stream=stream())
            _, unit, grp = H.composite_crc_batch(cod, c.sums, k, cell, C32C, bpc, data_len, want=("unit", "group"))
            # one rebuilt byte flipped (the first lost unit with a byte in the last stripe)
            res2 = bad2 = target = None
            live = [u for u in lost if c.lens[S - 1][u]]
            if live:
                target = live[0]
                cells2 = c.cells.clone()
                cells2[S - 1, target, c.lens[S - 1][target] - 1] ^= 0x40
                width = cells2.shape[2]
                ptrs2 = [cells2.data_ptr() + i * width for i in range(n)]
                res2, bad2 = prefilled(S, dev), torch.zeros((S, n), dtype=torch.uint8, device=dev)
                cod.scrub_crc_rows_device(ptrs2, strides, cell, S, c.sums.data_ptr(), bad2.data_ptr(),
                                          res2.data_ptr(), data_len=data_len, stream=stream())
            runs.append((c, data_len, res, bad, unit, grp, target, res2, bad2, cells2 if live else None))
    torch.cuda.synchronize()
    for c, data_len, res, bad, unit, grp, target, res2, bad2, _ in runs:
        what = (c.rs[-1], c.losts[0])
        c.check(what)
        assert as_u64(res, S).tolist() == [[0, 0]] * S, (what, res.tolist())
        assert not bool(bad.any()), what
        units = [oracle_crc(clib(), C32C, np.concatenate([c.t[s, u, :c.lens[s][u]] for s in range(S)]))
                 for u in range(n)]
        data = np.ascontiguousarray(c.t[:, :k]).reshape(-1)[:data_len or S * k * cell]
        assert be32(unit) == units, what
        assert be32(grp)[0] == oracle_crc(clib(), C32C, data), what
        if target is not None:
            got = as_u64(res2, S)
            assert not got[:S - 1].any(), what
            assert H.scrub_verdict(int(got[S - 1, 0]), int(got[S - 1, 1]), n) == (H.HEC_SCRUB_LOCATED, target), what
            want_bad = np.zeros((S, n), dtype=np.uint8)
            want_bad[S - 1, target] = 1
            assert np.array_equal(bad2.cpu().numpy(), want_bad), what


# ---- 7. graph capture -----------------------------------------------------------------------------

def test_graph_capture_replay(dev):
    """The uniform rows repair, the uniform rows scrub and the composite fold
    captured on one side stream after an eager run, replayed twice on restored
    inputs."""
    k, m, n, S, cell, bpc = 6, 3, 9, 3, 9232, 512
    full = k * cell
    data_len = (S - 1) * full + 3 * cell + 513
    rs = [full] * (S - 1) + [data_len - (S - 1) * full]
    cod = coder(k, m)
    c = Case(cod, k, m, cell, rs, [(3, k)] * S, dev, expected="same")
    cells0, sums0 = c.cells.clone(), c.sums.clone()
    unit = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
    grp = torch.zeros((4,), dtype=torch.uint8, device=dev)
    cws = torch.empty(max(4, H.composite_crc_workspace_size(n, S)), dtype=torch.uint8, device=dev)
    res, bad = prefilled(S, dev), torch.zeros((S, n), dtype=torch.uint8, device=dev)
    ptrs, strides = c.ptr_args()[:2]

    def work():
        c.uniform()
        cod.scrub_crc_rows_device(ptrs, strides, cell, S, c.sums.data_ptr(), bad.data_ptr(), res.data_ptr(),
                                  data_len=data_len, stream=stream())
        cod.composite_crc_device(C32C, c.sums.data_ptr(), n, k, cell, S, bpc, data_len, 0, unit.data_ptr(),
                                 grp.data_ptr(), cws.data_ptr(), cws.numel(), stream())

    work()  # eager once, then captured
    torch.cuda.synchronize()
    c.check("eager")
    assert as_u64(res, S).tolist() == [[0, 0]] * S
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        work()
    units = [oracle_crc(clib(), C32C, np.concatenate([c.t[s, u, :c.lens[s][u]] for s in range(S)])) for u in range(n)]
    group = oracle_crc(clib(), C32C, np.ascontiguousarray(c.t[:, :k]).reshape(-1)[:data_len])
    for rep in range(2):
        c.cells.copy_(cells0)
        c.sums.copy_(sums0)
        unit.fill_(SENT)
        grp.fill_(SENT)
        res.fill_(-1)
        bad.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.check(("replay", rep))
        assert as_u64(res, S).tolist() == [[0, 0]] * S and not bool(bad.any()), rep
        assert be32(unit) == units and be32(grp)[0] == group, rep


# ---- 8. argument errors queue nothing ----------------------------------------------------------------

def test_argument_errors_queue_nothing(dev):
    k, m, n, S, cell = 6, 3, 9, 4, 9232
    cod = coder(k, m)
    full = k * cell
    rs = [full] * (S - 1) + [cell + 5]
    b = Batch("rs", k, m, cell, rs, dev, masks=[present_mask(n, (1,))] * S, corrupt=[(S - 1, 0, 0)])
    ptrs, strides = b.slots()
    need = cod.scrub_crc_rows_mixed_workspace_size(S)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    ep, bp, rp, wp = b.exp.data_ptr(), b.bad.data_ptr(), b.res.data_ptr(), ws.data_ptr()
    inval = H.HEC_ERR_INVALID_ARG

    def uni(ctype=C32C, data_len=b.data_len(), S_=S, e=ep, bd=bp, r=rp, bpc=512):
        return H.lib.hec_scrub_crc_rows_device(cod.handle, ctype, H._pp(ptrs), H._sp(strides), cell, S_, bpc, data_len,
                                               e, bd, r, stream())

    def mix(ctype=C32C, lens=rs, e=ep, bd=bp, r=rp, w=wp, wn=need, bpc=512):
        import ctypes
        masks = (ctypes.c_uint64 * S)(*b.masks)
        arr = (ctypes.c_uint64 * S)(*lens)
        return H.lib.hec_scrub_crc_rows_device_mixed(cod.handle, ctype, H._pp(ptrs), H._sp(strides), masks, arr, cell,
                                                     S, bpc, e, bd, r, w, wn, stream())

    assert uni(ctype=H.CHECKSUM_NULL) == inval and mix(ctype=H.CHECKSUM_NULL) == inval
    for S_, data_len in ((S, (S - 1) * full), (S, 1), (S, S * full + 1), (0, 5)):
        assert uni(S_=S_, data_len=data_len) == inval, (S_, data_len)
    assert mix(lens=[full + 1] + rs[1:]) == inval
    assert mix(w=None) == inval and mix(w=wp + 8, wn=need) == inval and mix(wn=need - 1) == inval
    assert uni(e=None) == inval and mix(e=None) == inval
    assert uni(bd=None) == inval and mix(bd=None) == inval
    assert uni(r=rp + 4) == inval and mix(r=rp + 4) == inval
    assert uni(bpc=0) == inval and mix(bpc=0) == inval
    torch.cuda.synchronize()
    b.unchanged()
    # and the calls as they should be made still work afterwards
    b.mixed(cod, ws=ws[:need])
    torch.cuda.synchronize()
    b.check("after the errors")
