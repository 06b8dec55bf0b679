"""Verified reconstruction of short stripes on the GPU:
hec_reconstruct_crc_rows_device (data_len: a short last stripe) and
hec_reconstruct_crc_rows_device_mixed (one length per stripe) -- the one-pass
gf_crc_rows<RowsRepair> kernel and the byte-wise gf_reconstruct_rows_bytes.
Ground truth is the CPU oracle throughout, as test_gpu_reconstruct_sums.py's
short_group builds it: random data cut at the length, the oracle's parity of
the zero-padded cells, the oracle's chunk sums of each unit's true bytes.  The
whole-buffer-image discipline of test_gpu_reconstruct_crc.py: 0xEE in every
slot byte at or past len(u), in lost slots and between cell_len and the
stride, 0xA5 in every sums byte, zeroed flags; after a call the ENTIRE cell
buffer, sums buffer and flag buffer must equal their expected images (only the
targets' [0, n0) and their live sums are free in a flagged stripe), so a read
of a byte past a unit's length, a write at or past n0 or to a dead sums slot
shows as well as a wrong byte."""
import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
from composite_crc_cases import data_len_cases, oracle_crc
from test_gpu_reconstruct_crc import GARBAGE, SENT, chunk_sums, coder, present_mask, slots, stream
from test_gpu_reconstruct_sums import be32, clib, short_losses

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
OUTFILL = 0xA5
GUARD = 0xC3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def unit_lens(k, n, cell, r):
    """len(u) of every unit of a stripe of r logical bytes (the issue's geometry)."""
    n0 = min(cell, r)
    return [min(cell, max(0, r - u * cell)) if u < k else n0 for u in range(n)]


_cells = {}
_sums = {}


def stripes_truth(k, m, cell, rs, seed=0):
    """The true stripes of a batch whose stripe s holds rs[s] logical bytes,
    once per batch, read-only: cells [S, n, cell] (random data up to rs[s],
    zeros behind it, the oracle's parity of that) and lens [S][n]."""
    key = (k, m, cell, tuple(rs), seed)
    if key not in _cells:
        S, n = len(rs), k + m
        rng = np.random.default_rng(1000 * k + cell + 7 * sum(rs) + seed)
        data = rng.integers(0, 256, size=(S, k * cell), dtype=np.uint8)
        for s, r in enumerate(rs):
            data[s, r:] = 0
        t = np.zeros((S, n, cell), dtype=np.uint8)
        t[:, :k] = data.reshape(S, k, cell)
        par = O.matmul_shards(O.codec_matrix("rs", k, m)[k:], [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)])
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        t.setflags(write=False)
        _cells[key] = (t, [unit_lens(k, n, cell, r) for r in rs])
    return _cells[key]


def stripes_sums(k, m, cell, rs, bpc, ctype, seed=0):
    """The oracle's chunk sums of every unit's true bytes: [S, n, nck, 4], SENT
    where no live chunk is."""
    key = (k, m, cell, tuple(rs), bpc, ctype, seed)
    if key not in _sums:
        t, lens = stripes_truth(k, m, cell, rs, seed)
        S, n = len(rs), k + m
        sums = np.full((S, n, -(-cell // bpc), 4), SENT, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if lens[s][u]:
                    live = chunk_sums(t[s, u, :lens[s][u]], bpc, ctype)
                    sums[s, u, :live.shape[0]] = live
        sums.setflags(write=False)
        _sums[key] = sums
    return _sums[key]


def forget_truth(k, m, cell, rs):
    """Drops what stripes_truth and stripes_sums keep of one batch (a large
    batch holds over 100 MB)."""
    for cache in (_cells, _sums):
        for key in [key for key in cache if key[:4] == (k, m, cell, tuple(rs))]:
            del cache[key]


def forget(min_bytes):
    """Drops the cached batches of at least min_bytes of cells, with their sums."""
    for key in [key for key, v in _cells.items() if v[0].nbytes >= min_bytes]:
        forget_truth(*key[:4])


class Case:
    """One call's buffers and their expected images.

    rs[s] = the logical bytes of stripe s; losts[s] = the units stripe s lacks,
    wants[s] = those to rebuild (None: all of them).  corrupt = [(stripe, unit,
    byte)]: that slot byte of a present cell is flipped (a byte at or past the
    unit's length is the caller's garbage and must change nothing);
    corrupt_sums = [(stripe, unit, chunk)]: that expected sum instead.
    expected: "sep" / "same" / None and separate / base_off / pad as
    test_gpu_reconstruct_crc.Case.  zero_pad: the present slots hold zeros
    from len(u) up to n0, as a reader pads them (what a scrub of the stripe
    needs), where they otherwise hold 0xEE."""

    def __init__(self, cod, k, m, cell, rs, losts, dev, wants=None, expected="sep", corrupt=(), corrupt_sums=(), pad=0,
                 separate=False, base_off=0, bpc=512, ctype=C32C, seed=0, zero_pad=False):
        t, lens = stripes_truth(k, m, cell, rs, seed)
        true = stripes_sums(k, m, cell, rs, bpc, ctype, seed)
        S, n = len(rs), k + m
        self.cod, self.S, self.n, self.k, self.cell, self.bpc, self.ctype = cod, S, n, k, cell, bpc, ctype
        self.rs, self.lens, self.t = list(rs), lens, t
        self.losts = [tuple(l) for l in losts]
        self.wants = [tuple(l) for l in losts] if wants is None else [tuple(w) for w in wants]
        self.have_want = wants is not None
        width = cell + pad
        host = np.full((S, n, width), GARBAGE, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if u not in self.losts[s]:
                    if zero_pad:
                        host[s, u, :min(cell, self.rs[s])] = 0
                    host[s, u, :lens[s][u]] = t[s, u, :lens[s][u]]
        for (s, u, b) in corrupt:
            assert u not in self.losts[s]
            host[s, u, b] ^= 0x40
        exp_host = host.copy()
        out_host = np.full((S, n, width), OUTFILL, dtype=np.uint8)
        for s in range(S):
            n0 = min(cell, self.rs[s])
            for u in self.wants[s]:
                dst = out_host if separate else exp_host
                dst[s, u, :n0] = 0
                dst[s, u, :lens[s][u]] = t[s, u, :lens[s][u]]
        self.raw = torch.full((S * n * width + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = self.raw[base_off:].view(S, n, width)
        self.cells.copy_(torch.from_numpy(host).to(dev))
        self.exp_cells = torch.from_numpy(exp_host).to(dev)
        self.out = self.exp_out = None
        if separate:
            self.out = torch.full((S, n, width), OUTFILL, dtype=torch.uint8, device=dev)
            self.exp_out = torch.from_numpy(out_host).to(dev)
        self.ts = torch.from_numpy(true.copy()).to(dev)  # [S, n, nck, 4], SENT past the live chunks
        self.sums = torch.full(tuple(self.ts.shape), SENT, dtype=torch.uint8, device=dev)
        self.expected = None
        if expected == "sep":
            self.expected = self.ts.clone()
        elif expected == "same":
            for s, lost in enumerate(self.losts):
                keep = [i for i in range(n) if i not in lost]
                self.sums[s, keep] = self.ts[s, keep]
            self.expected = self.sums
        if expected is not None:
            for (s, u, c) in corrupt_sums:
                assert u not in self.losts[s] and c < -(-lens[s][u] // bpc)
                self.expected[s, u, c, 3] ^= 1
        self.exp_sums = self.sums.clone()
        for s, w in enumerate(self.wants):
            for i in w:
                self.exp_sums[s, i] = self.ts[s, i]
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        self.exp_bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        self.dirty = set()
        hits = [(s, u) for (s, u, b) in corrupt if b < lens[s][u]]
        hits += [(s, u) for (s, u, _) in corrupt_sums] if expected is not None else []
        for (s, u) in hits:
            surv = [i for i in range(n) if i not in self.losts[s]][:k]
            if u in surv and self.wants[s]:
                self.dirty.add(s)
                if expected is not None:
                    self.exp_bad[s, u] = 1

    def ptr_args(self):
        ptrs, strides = slots(self.cells)
        optrs, ostrides = slots(self.out) if self.out is not None else (ptrs, strides)
        return ptrs, strides, optrs, ostrides

    def chk_args(self):
        return dict(expected_ptr=None if self.expected is None else self.expected.data_ptr(),
                    bad_ptr=None if self.expected is None else self.bad.data_ptr(),
                    bytes_per_checksum=self.bpc, checksum_type=self.ctype)

    def data_len(self):
        """The uniform form's data_len: only the last stripe may be short."""
        full = self.k * self.cell
        assert all(r == full for r in self.rs[:-1])
        return 0 if self.rs[-1] == full else (self.S - 1) * full + self.rs[-1]

    def uniform(self, strm=None, data_len=None):
        assert len(set(self.losts)) == 1 and len(set(self.wants)) == 1
        ptrs, strides, optrs, ostrides = self.ptr_args()
        shards = [None if i in self.losts[0] else ptrs[i] for i in range(self.n)]
        self.cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, self.cell, self.S, self.sums.data_ptr(),
                                             want=list(self.wants[0]) if self.have_want else None,
                                             data_len=self.data_len() if data_len is None else data_len,
                                             stream=stream() if strm is None else strm, **self.chk_args())

    def mixed(self, workspace=None, strm=None, stripe_bytes="rs"):
        ptrs, strides, optrs, ostrides = self.ptr_args()
        masks = [present_mask(self.n, l) for l in self.losts]
        wants = [sum(1 << i for i in w) for w in self.wants] if self.have_want else None
        if workspace is None:
            workspace = torch.empty(self.cod.reconstruct_crc_rows_mixed_workspace_size(self.S), dtype=torch.uint8,
                                    device=self.cells.device)
        self.workspace = workspace
        self.cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, masks, wants,
                                                   self.rs if stripe_bytes == "rs" else stripe_bytes, self.cell,
                                                   self.S, self.sums.data_ptr(), workspace.data_ptr(),
                                                   workspace.numel(), stream=stream() if strm is None else strm,
                                                   **self.chk_args())

    def check(self, what=""):
        """After a synchronize: everything equals its expected image; in a
        stripe that read a corrupt survivor the targets' [0, n0) and their live
        sums are unspecified, everything else still holds."""
        assert torch.equal(self.bad, self.exp_bad), (what, "flags", self.bad.nonzero().tolist(),
                                                     self.exp_bad.nonzero().tolist())
        bufs = [("cells", self.cells, self.exp_cells)]
        if self.out is not None:
            bufs.append(("out", self.out, self.exp_out))
        sums, exp_sums = self.sums, self.exp_sums
        if self.dirty:
            bufs = [(name, g.clone(), e.clone()) for name, g, e in bufs]
            sums, exp_sums = sums.clone(), exp_sums.clone()
            for s in self.dirty:
                n0 = min(self.cell, self.rs[s])
                for i in self.wants[s]:
                    live = -(-self.lens[s][i] // self.bpc)
                    sums[s, i, :live] = 0
                    exp_sums[s, i, :live] = 0
                    for _, g, e in bufs:
                        g[s, i, :n0] = 0
                        e[s, i, :n0] = 0
        for name, g, e in bufs + [("sums", sums, exp_sums)]:
            if not torch.equal(g, e):
                ne = (g != e).reshape(g.shape[0], g.shape[1], -1)
                diff = ne.any(dim=2).nonzero().tolist()
                first = ne[diff[0][0], diff[0][1]].nonzero()[0].item()
                raise AssertionError((what, name, "stripe/unit pairs that differ", diff[:20], "first offset", first,
                                      "lens", self.lens[diff[0][0]]))

    def no_change(self, what=""):
        assert not bool(self.bad.any()), what
        assert torch.equal(self.cells, self.exp_cells) or self.out is None, what
        assert bool((self.sums == SENT).all()) or self.expected is self.sums, what
        if self.out is not None:
            assert bool((self.out == OUTFILL).all()), what


def cut_lengths(k, cell, tile):
    """r of the short stripe: cuts that leave the cut unit (a middle one) with
    1, 15, 16, 17, 511, 512, 513 and cell-1 bytes and with a length inside the
    second block tile; r < cell_len (parity short, data units 1.. empty) and
    r == cell_len."""
    cu = max(1, k // 2)
    xs = [1, 15, 16, 17, 511, 512, 513, cell - 1]
    if tile + 4321 < cell:
        xs.append(tile + 4321)
    return [cu * cell + x for x in xs] + [777, cell]


def last_short(k, cell, S, data_len):
    full = k * cell
    return [full] * (S - 1) + [(data_len or S * full) - (S - 1) * full]


# ---- 1. short last stripe, fused shapes ---------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("cell", [9232, 50192])
@pytest.mark.parametrize("k,m", [(6, 3), (3, 2), (10, 4), (2, 1)])
def test_short_last_stripe_fused_shapes(dev, k, m, cell, ctype):
    """gf_crc_rows<RowsRepair> behind the full stripes' gf_reconstruct_crc:
    every length, short_losses' five losses per length, d_expected absent /
    separate / the sums array, out of place and in place, by rotation."""
    S = 3
    cod = coder(k, m)
    full = k * cell
    tile = 32768 if k <= 6 else 16384
    lengths = [dl for dl in data_len_cases(k, cell, S)] + [(S - 1) * full + r for r in cut_lengths(k, cell, tile)]
    cases = []
    for li, data_len in enumerate(dict.fromkeys(lengths)):
        rs = last_short(k, cell, S, data_len)
        for ci, lost in enumerate(short_losses(k, m, cell, S, data_len)):
            if any(u >= k + m for u in lost) or len(set(lost)) != len(lost) or len(lost) > m:
                continue
            c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected=(None, "sep", "same")[(li + ci) % 3], pad=48,
                     separate=(li + ci // 3) % 2 == 0, ctype=ctype)
            assert c.data_len() == (0 if data_len in (0, S * full) else data_len)
            c.uniform()
            cases.append(c)
    torch.cuda.synchronize()
    assert len(cases) >= 40
    for c in cases:
        assert not c.dirty
        c.check((c.rs[-1], c.losts[0], c.expected is not None, c.out is not None))


# ---- 2. the byte-wise route ---------------------------------------------------------

@pytest.mark.parametrize("shape", ["rs42", "bpc1024", "bpc100", "base1", "cell528", "cell1000", "rs65"])
def test_bytewise_route(dev, shape):
    """The shapes the one-pass kernel does not take run gf_reconstruct_rows_bytes
    behind the full stripes' composition: same images."""
    k, m, cell, kw, losses = 6, 3, 9232, {}, None
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
    S, full = 3, k * cell
    cod = coder(k, m)
    cu = max(1, k // 2)
    lengths = data_len_cases(k, cell, S) + [(S - 1) * full + r
                                            for r in (cu * cell + 1, cu * cell + 17, cu * cell + cell - 1, 77, cell)]
    cases = []
    for li, data_len in enumerate(dict.fromkeys(lengths)):
        rs = last_short(k, cell, S, data_len)
        losses = [(1, 3, 6, 8, 10)] if shape == "rs65" else short_losses(k, m, cell, S, data_len)
        for ci, lost in enumerate(losses):
            if len(lost) > m:
                continue
            c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected=(None, "sep", "same")[(li + ci) % 3], pad=7,
                     separate=(li + ci // 3) % 2 == 0, ctype=(C32C, C32)[li % 2], **kw)
            c.uniform()
            cases.append(c)
    if shape == "base1":
        assert cases[0].cells.data_ptr() % 16 == 1
    torch.cuda.synchronize()
    for c in cases:
        c.check((shape, c.rs[-1], c.losts[0], c.expected is not None, c.out is not None))


# ---- 3. flags -----------------------------------------------------------------------

@pytest.mark.parametrize("k,m,cell,bpc", [(6, 3, 9232, 512), (10, 4, 9232, 512), (6, 3, 1000, 100)])
def test_flags_in_the_short_stripe(dev, k, m, cell, bpc):
    """A flipped byte inside a survivor's own bytes of the short stripe, a
    flipped expected sum of its short last chunk: exactly that flag.  A flipped
    slot byte at len(u) of the cut unit: no flag and no change."""
    S, full = 3, k * cell
    cu = max(1, k // 2)
    x = 513 if bpc == 512 else 317  # the cut unit's bytes: a short last chunk
    rs = [full] * (S - 1) + [cu * cell + x]
    lost = (0,)
    cod = coder(k, m)
    runs = []
    for expected in ("sep", "same"):
        runs.append(Case(cod, k, m, cell, rs, [lost] * S, dev, expected=expected, bpc=bpc,
                         corrupt=[(S - 1, cu, x - 1)]))
        runs.append(Case(cod, k, m, cell, rs, [lost] * S, dev, expected=expected, bpc=bpc,
                         corrupt=[(S - 1, 1, cell // 2)]))
        runs.append(Case(cod, k, m, cell, rs, [lost] * S, dev, expected=expected, bpc=bpc,
                         corrupt_sums=[(S - 1, cu, (x - 1) // bpc)]))
        clean = Case(cod, k, m, cell, rs, [lost] * S, dev, expected=expected, bpc=bpc, corrupt=[(S - 1, cu, x)])
        assert not clean.dirty and int(clean.exp_bad.sum()) == 0
        runs.append(clean)
    for i, c in enumerate(runs):
        c.mixed() if i in (2, 5) else c.uniform()
    torch.cuda.synchronize()
    for i, c in enumerate(runs):
        if i % 4 != 3:
            assert c.dirty == {S - 1} and int(c.exp_bad.sum()) == 1
        c.check(i)


# ---- 4. one pattern and one length per stripe ---------------------------------------

def mixed_batch(k, m, cell, tile, S=24):
    n, full = k + m, k * cell
    rs_cycle = [0, full, 1, cell, cell + 1] + cut_lengths(k, cell, tile)
    rs, losts, wants = [], [], []
    for s in range(S):
        r = rs_cycle[(7 * s + 3) % len(rs_cycle)]
        rs.append(r)
        if s in (5, 17):
            lost = w = ()
        elif s == 11:
            lost = (1, k)
            w = lost
        elif s % 6 == 4:
            lost = (s % n, (s + 3) % n)
            w = (lost[s % 2],)  # narrower than the loss
        else:
            lost = w = (s % n,)
        losts.append(tuple(sorted(lost)))
        wants.append(tuple(sorted(w)))
    return rs, losts, wants


@pytest.mark.parametrize("route", ["fused", "bytes"])
@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_lengths_and_patterns(dev, k, m, route):
    """24 stripes, per-stripe masks and lengths; the workspace of exactly the
    advertised size keeps its guard bands."""
    cell = 9232 if route == "fused" else 1000
    bpc = 512 if route == "fused" else 100
    rs, losts, wants = mixed_batch(k, m, cell, 32768 if k <= 6 else 16384)
    S = len(rs)
    full = k * cell
    true_rs = [r or full for r in rs]
    cod = coder(k, m)
    nbytes = cod.reconstruct_crc_rows_mixed_workspace_size(S)
    buf = torch.full((nbytes + 512,), GUARD, dtype=torch.uint8, device=dev)
    ws = buf[256:256 + nbytes]
    assert ws.data_ptr() % 8 == 0
    a = Case(cod, k, m, cell, true_rs, losts, dev, wants=wants, expected="same", pad=16, bpc=bpc)
    a.mixed(workspace=ws, stripe_bytes=rs)
    b = Case(cod, k, m, cell, true_rs, losts, dev, wants=wants, expected=None, separate=True, bpc=bpc, ctype=C32)
    b.mixed(stripe_bytes=rs)
    c = Case(cod, k, m, cell, true_rs, losts, dev, wants=None, expected="sep", bpc=bpc)
    c.mixed(stripe_bytes=rs)
    torch.cuda.synchronize()
    a.check("want, same")
    b.check("want, separate")
    c.check("all")
    assert bool((buf[:256] == GUARD).all()) and bool((buf[256 + nbytes:] == GUARD).all())


def test_tensor_helper(dev):
    k, m, cell = 6, 3, 9232
    rs, losts, _ = mixed_batch(k, m, cell, 32768)
    cod = coder(k, m)
    c = Case(cod, k, m, cell, [r or k * cell for r in rs], losts, dev, expected="same")
    ws = H.reconstruct_crc_rows_batch_mixed(cod, c.cells, [present_mask(k + m, l) for l in losts], c.sums,
                                            stripe_bytes=rs, expected=c.sums, bad=c.bad)
    assert ws.numel() == cod.reconstruct_crc_rows_mixed_workspace_size(len(rs))
    torch.cuda.synchronize()
    c.check()


# ---- 5. identity with the full-stripe calls -----------------------------------------

@pytest.mark.parametrize("cell", [9232, 1000])
def test_full_stripes_identical_to_reconstruct_crc(dev, cell):
    """data_len == 0 and stripe_bytes NULL / all zero / all k*cell_len: cells,
    sums and flags byte-identical to hec_reconstruct_crc_device[_mixed]."""
    k, m, n, S = 6, 3, 9, 9
    cod = coder(k, m)
    full = k * cell
    from test_gpu_reconstruct_crc import mixed_case, uniform_case
    kw = dict(corrupt_sums=[(1, 0, 0), (7, 5, (cell - 1) // 512)])
    ref = uniform_case(cod, k, m, S, cell, (2, 6), dev, **kw)
    ref.uniform()
    got = uniform_case(cod, k, m, S, cell, (2, 6), dev, **kw)
    ptrs, strides, optrs, ostrides = got.ptr_args()
    shards = [None if i in (2, 6) else ptrs[i] for i in range(n)]
    got.cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, S, got.sums.data_ptr(), data_len=0,
                                        stream=stream(), **got.chk_args())
    pairs = [(ref, got)]
    losts = [((s % n,), (s % n, (s + 4) % n), ())[s % 3] for s in range(S)]
    mref = mixed_case(cod, k, m, S, cell, losts, dev, **kw)
    mref.mixed()
    for sb in (None, [0] * S, [full] * S, [0, full] * (S // 2) + [0]):
        g = mixed_case(cod, k, m, S, cell, losts, dev, **kw)
        ptrs, strides, optrs, ostrides = g.ptr_args()
        ws = torch.empty(cod.reconstruct_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, [present_mask(n, l) for l in losts],
                                              None, sb, cell, S, g.sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                              stream=stream(), **g.chk_args())
        g.workspace = ws
        pairs.append((mref, g))
    torch.cuda.synchronize()
    assert int(ref.bad.sum()) >= 1
    for i, (r, g) in enumerate(pairs):
        assert torch.equal(r.cells, g.cells), i
        assert torch.equal(r.sums, g.sums), i
        assert torch.equal(r.bad, g.bad), i


# ---- 6. then the composite ----------------------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (3, 2, 528), (4, 2, 1000)])
def test_rows_then_composite(dev, k, m, cell, ctype):
    """In-place rows call with d_expected == d_sums, then
    hec_composite_crc_device with the same data_len on the same stream: the
    oracle's CRC of each unit's actual bytes and of the file."""
    n, S, bpc = k + m, 3, 512
    cod = coder(k, m)
    runs = []
    for data_len in data_len_cases(k, cell, S):
        rs = last_short(k, cell, S, data_len)
        for lost in short_losses(k, m, cell, S, data_len):
            if len(lost) > m:
                continue
            c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected="same", ctype=ctype)
            c.uniform(data_len=data_len)
            _, unit, grp = H.composite_crc_batch(cod, c.sums, k, cell, ctype, bpc, data_len, want=("unit", "group"))
            runs.append((c, data_len, unit, grp))
    torch.cuda.synchronize()
    for c, data_len, unit, grp in runs:
        c.check((data_len, c.losts[0]))
        units = [oracle_crc(clib(), ctype, np.concatenate([c.t[s, u, :c.lens[s][u]] for s in range(S)]))
                 for u in range(n)]
        data = np.ascontiguousarray(c.t[:, :k]).reshape(-1)[:data_len or S * k * cell]
        assert be32(unit) == units, (data_len, c.losts[0])
        assert be32(grp)[0] == oracle_crc(clib(), ctype, data), (data_len, c.losts[0])


# ---- 7. the repair loop on a short group --------------------------------------------

@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (10, 4, 9232), (4, 2, 1000)])
def test_repair_then_scrub(dev, k, m, cell):
    """Rows call in place, then hec_scrub_device over the full stripes and
    over the last stripe with cell_len = n0: every pair (0, 0)."""
    n, S = k + m, 4
    cod = coder(k, m)
    full = k * cell
    runs = []
    for r in (1, 777, cell, cell + 17, max(1, k // 2) * cell + 513, full - 1):
        rs = [full] * (S - 1) + [r]
        for lost in ((0,), (max(1, k // 2), k), (k - 1, n - 1)):
            if len(lost) > m:
                continue
            c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected="same", zero_pad=True)
            c.uniform()
            res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
            ptrs, strides = slots(c.cells)
            cod.scrub_device(ptrs, strides, cell, S - 1, res.data_ptr(), stream())
            n0 = min(cell, r)
            last = [p + (S - 1) * strides[0] for p in ptrs]
            cod.scrub_device(last, strides, n0, 1, res[S - 1:].data_ptr(), stream())
            runs.append((c, res))
    torch.cuda.synchronize()
    for c, res in runs:
        c.check((c.rs[-1], c.losts[0]))
        assert res.tolist() == [[0, 0]] * S, (c.rs[-1], c.losts[0], res.tolist())


# ---- 8. graph -----------------------------------------------------------------------

def test_graph_capture_replay_with_composite(dev):
    """The uniform form and hec_composite_crc_device captured on one stream and
    replayed twice on fresh sentinel-filled outputs."""
    k, m, n, S, cell, bpc = 6, 3, 9, 3, 9232, 512
    data_len = (S - 1) * k * cell + 3 * cell + 513
    rs = last_short(k, cell, S, data_len)
    cod = coder(k, m)
    lost = (3, k)
    c = Case(cod, k, m, cell, rs, [lost] * S, dev, expected="same")
    cells0, sums0 = c.cells.clone(), c.sums.clone()
    unit = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
    grp = torch.zeros((4,), dtype=torch.uint8, device=dev)
    cws = torch.empty(max(4, H.composite_crc_workspace_size(n, S)), dtype=torch.uint8, device=dev)
    c.uniform()  # eager once, then captured
    torch.cuda.synchronize()
    c.check("eager")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.uniform()
        cod.composite_crc_device(C32C, c.sums.data_ptr(), n, k, cell, S, bpc, data_len, 0, unit.data_ptr(),
                                 grp.data_ptr(), cws.data_ptr(), cws.numel(), stream())
    units = [oracle_crc(clib(), C32C, np.concatenate([c.t[s, u, :c.lens[s][u]] for s in range(S)])) for u in range(n)]
    group = oracle_crc(clib(), C32C, np.ascontiguousarray(c.t[:, :k]).reshape(-1)[:data_len])
    for rep in range(2):
        c.cells.copy_(cells0)
        c.sums.copy_(sums0)
        unit.fill_(SENT)
        grp.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.check(("replay", rep))
        assert be32(unit) == units, rep
        assert be32(grp)[0] == group, rep


# ---- argument errors on the device, nothing queued -----------------------------------

def test_argument_errors_write_nothing(dev):
    k, m, n, S, cell = 6, 3, 9, 4, 9232
    cod = coder(k, m)
    full = k * cell
    rs = [full] * (S - 1) + [cell + 5]
    c = Case(cod, k, m, cell, rs, [(1, 7)] * S, dev, expected="sep", separate=True)
    ptrs, strides, optrs, ostrides = c.ptr_args()
    shards = [None if i in (1, 7) else ptrs[i] for i in range(n)]
    masks = [present_mask(n, (1, 7))] * S
    ws = torch.empty(cod.reconstruct_crc_rows_mixed_workspace_size(S) + 16, dtype=torch.uint8, device=dev)
    sp, wp, wn = c.sums.data_ptr(), ws.data_ptr(), ws.numel()

    def both(**kw):
        sums_ptr = kw.pop("sums_ptr", sp)
        with pytest.raises(ValueError):
            cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, S, sums_ptr, data_len=c.data_len(),
                                            stream=stream(), **kw)
        with pytest.raises(ValueError):
            cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, masks, None, rs, cell, S, sums_ptr,
                                                  wp, wn, stream=stream(), **kw)

    both(checksum_type=H.CHECKSUM_NULL)
    both(checksum_type=7)
    both(bytes_per_checksum=0)
    both(sums_ptr=None)
    both(sums_ptr=sp + 2)
    both(expected_ptr=c.expected.data_ptr(), bad_ptr=None)
    for S_, data_len in ((S, (S - 1) * full), (S, 1), (S, S * full + 1), (0, 5)):
        with pytest.raises(ValueError):
            cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, S_, sp, data_len=data_len,
                                            stream=stream())
    with pytest.raises(ValueError):
        cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, masks, None, [full + 1] + rs[1:], cell,
                                              S, sp, wp, wn, stream=stream())
    # a want bit on a present unit; a target without storage
    with pytest.raises(ValueError):
        cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, S, sp, want=[0],
                                        data_len=c.data_len(), stream=stream())
    with pytest.raises(ValueError):
        cod.reconstruct_crc_rows_device(shards, strides, [None if i == 7 else p for i, p in enumerate(optrs)],
                                        ostrides, cell, S, sp, data_len=c.data_len(), stream=stream())
    # fewer than k units present
    with pytest.raises(H.ErasureCodingError):
        cod.reconstruct_crc_rows_device([None] * 4 + ptrs[4:], strides, optrs, ostrides, cell, S, sp,
                                        data_len=c.data_len(), stream=stream())
    with pytest.raises(H.ErasureCodingError):
        cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides,
                                              masks[:-1] + [present_mask(n, (1, 2, 7, 8))], None, rs, cell, S, sp, wp,
                                              wn, stream=stream())
    # a workspace that is too small, NULL or misaligned
    for p, nbytes in ((wp, cod.reconstruct_crc_mixed_workspace_size(S)), (wp, 64), (None, wn), (wp + 4, wn - 4)):
        with pytest.raises(ValueError):
            cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, masks, None, rs, cell, S, sp, p,
                                                  nbytes, stream=stream())
    torch.cuda.synchronize()
    c.no_change()
    # no stripes, or no target anywhere: OK, and still nothing written
    cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, 0, sp, stream=stream())
    cod.reconstruct_crc_rows_device(shards, strides, optrs, ostrides, cell, S, sp, want=[], data_len=c.data_len(),
                                    stream=stream())
    cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, [], None, [], cell, 0, sp, wp, wn,
                                          stream=stream())
    cod.reconstruct_crc_rows_device_mixed(ptrs, strides, optrs, ostrides, masks, [0] * S, rs, cell, S, sp, wp, wn,
                                          stream=stream())
    torch.cuda.synchronize()
    c.no_change()
