"""Encode with chunk sums of short stripes on the GPU:
hec_encode_crc_rows_device (data_len: a short last stripe) and
hec_encode_crc_rows_device_mixed (one length per stripe) -- the one-pass
gf_crc_rows<RowsEncode> kernel and the byte-wise gf_encode_rows_bytes.  Ground truth
is the CPU oracle throughout: random data cut at the length, the oracle's parity
(O.codec_matrix(codec, k, m)[k:]) of the zero-padded cells, the oracle's chunk
sums of each unit's true bytes.  The whole-buffer-image discipline of
test_gpu_reconstruct_crc_rows.py: the data slots hold 0xEE at and past len(u)
and between cell_len and the stride, the parity slots are pre-filled 0xA5, the
sums array with the sentinel; after a call the ENTIRE cell buffer (data and
parity slots) and sums buffer must equal their expected images, so a read of a
byte past a unit's length, a write at or past n0 or to a dead sums slot shows as
well as a wrong byte."""
import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
from composite_crc_cases import data_len_cases, oracle_crc
from test_gpu_reconstruct_crc import GARBAGE, SENT, chunk_sums, coder, slots, stream
from test_gpu_reconstruct_crc_rows import cut_lengths, last_short, unit_lens
from test_gpu_reconstruct_sums import be32, clib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
OUTFILL = 0xA5
GUARD = 0xC3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_cells = {}
_sums = {}


def stripes_truth(codec, k, m, cell, rs, seed=0):
    """The true stripes of a batch whose stripe s holds rs[s] logical bytes,
    once per batch, read-only: cells [S, n, cell] (random data up to rs[s],
    zeros behind it, the oracle's parity of that) and lens [S][n]."""
    key = (codec, k, m, cell, tuple(rs), seed)
    if key not in _cells:
        S, n = len(rs), k + m
        rng = np.random.default_rng(1000 * k + cell + 7 * sum(rs) + seed)
        data = rng.integers(0, 256, size=(S, k * cell), dtype=np.uint8)
        for s, r in enumerate(rs):
            data[s, r:] = 0
        t = np.zeros((S, n, cell), dtype=np.uint8)
        t[:, :k] = data.reshape(S, k, cell)
        par = O.matmul_shards(O.codec_matrix(codec, k, m)[k:],
                              [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)])
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        t.setflags(write=False)
        _cells[key] = (t, [unit_lens(k, n, cell, r) for r in rs])
    return _cells[key]


def stripes_sums(codec, k, m, cell, rs, bpc, ctype, seed=0):
    """The oracle's chunk sums of every unit's true bytes: [S, n, nck, 4], SENT
    where no live chunk is."""
    key = (codec, k, m, cell, tuple(rs), bpc, ctype, seed)
    if key not in _sums:
        t, lens = stripes_truth(codec, k, m, cell, rs, seed)
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


def forget(min_bytes):
    """Drops the cached batches of at least min_bytes of cells, with their sums."""
    for key in [key for key, v in _cells.items() if v[0].nbytes >= min_bytes]:
        del _cells[key]
        for other in [o for o in _sums if o[:5] == key[:5] and o[-1] == key[-1]]:
            del _sums[other]


class Enc:
    """One call's buffers and their expected images.  rs[s] = the logical bytes
    of stripe s (never 0 here).  The cell buffer is [S, k+m, cell + pad]: units
    below k are the data slots (true bytes below len(u), 0xEE behind), the
    others the parity slots (0xA5).  base_off moves its base off the 16-B grid."""

    def __init__(self, cod, k, m, cell, rs, dev, codec="rs", pad=48, base_off=0, bpc=512, ctype=C32C, seed=0):
        t, lens = stripes_truth(codec, k, m, cell, rs, seed)
        true = stripes_sums(codec, k, m, cell, rs, bpc, ctype, seed)
        S, n = len(rs), k + m
        self.cod, self.S, self.n, self.k, self.m, self.cell, self.bpc, self.ctype = cod, S, n, k, m, cell, bpc, ctype
        self.rs, self.lens, self.t = list(rs), lens, t
        width = cell + pad
        host = np.full((S, n, width), GARBAGE, dtype=np.uint8)
        host[:, k:] = OUTFILL
        for s in range(S):
            for u in range(k):
                host[s, u, :lens[s][u]] = t[s, u, :lens[s][u]]
        exp_host = host.copy()
        for s in range(S):
            n0 = min(cell, self.rs[s])
            exp_host[s, k:, :n0] = t[s, k:, :n0]
        self.host = host
        self.raw = torch.full((S * n * width + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = self.raw[base_off:].view(S, n, width)
        self.cells.copy_(torch.from_numpy(host).to(dev))
        self.exp_cells = torch.from_numpy(exp_host).to(dev)
        self.exp_sums = torch.from_numpy(true.copy()).to(dev)  # [S, n, nck, 4], SENT past the live chunks
        self.sums = torch.full(tuple(self.exp_sums.shape), SENT, dtype=torch.uint8, device=dev)

    def reset(self):
        """Inputs and sentinel-filled outputs again."""
        self.cells.copy_(torch.from_numpy(self.host).to(self.cells.device))
        self.sums.fill_(SENT)

    def ptr_args(self):
        ptrs, strides = slots(self.cells)
        k = self.k
        return ptrs[:k], strides[:k], ptrs[k:], strides[k:]

    def kw(self):
        return dict(bytes_per_checksum=self.bpc, checksum_type=self.ctype)

    def data_len(self):
        """The uniform form's data_len: only the last stripe may be short."""
        full = self.k * self.cell
        assert all(r == full for r in self.rs[:-1])
        return 0 if self.rs[-1] == full else (self.S - 1) * full + self.rs[-1]

    def uniform(self, data_len=None, strm=None):
        dp, ds, pp, ps = self.ptr_args()
        self.cod.encode_crc_rows_device(dp, ds, pp, ps, self.cell, self.S, self.sums.data_ptr(),
                                        data_len=self.data_len() if data_len is None else data_len,
                                        stream=stream() if strm is None else strm, **self.kw())

    def mixed(self, stripe_bytes="rs", workspace=None):
        dp, ds, pp, ps = self.ptr_args()
        if workspace is None:
            workspace = torch.empty(max(8, self.cod.encode_crc_rows_mixed_workspace_size(self.S)), dtype=torch.uint8,
                                    device=self.cells.device)
        self.workspace = workspace
        self.cod.encode_crc_rows_device_mixed(dp, ds, pp, ps, self.rs if stripe_bytes == "rs" else stripe_bytes,
                                              self.cell, self.S, self.sums.data_ptr(), workspace.data_ptr(),
                                              workspace.numel(), stream=stream(), **self.kw())

    def check(self, what=""):
        """After a synchronize: everything equals its expected image."""
        for name, g, e in (("cells", self.cells, self.exp_cells), ("sums", self.sums, self.exp_sums)):
            if not torch.equal(g, e):
                ne = (g != e).reshape(g.shape[0], g.shape[1], -1)
                diff = ne.any(dim=2).nonzero().tolist()
                first = ne[diff[0][0], diff[0][1]].nonzero()[0].item()
                raise AssertionError((what, name, "stripe/unit pairs that differ", diff[:20], "first offset", first,
                                      "lens", self.lens[diff[0][0]]))

    def no_change(self, what=""):
        assert torch.equal(self.cells, torch.from_numpy(self.host).to(self.cells.device)), what
        assert bool((self.sums == SENT).all()), what

    def crcs(self, data_len):
        """The oracle's CRC of each unit's actual bytes and of the file bytes."""
        S, n, k = self.S, self.n, self.k
        units = [oracle_crc(clib(), self.ctype, np.concatenate([self.t[s, u, :self.lens[s][u]] for s in range(S)]))
                 for u in range(n)]
        data = np.ascontiguousarray(self.t[:, :k]).reshape(-1)[:data_len or S * k * self.cell]
        return units, oracle_crc(clib(), self.ctype, data)


def tile_of(k):
    return 32768 if k <= 6 else 16384


# ---- 1. short last stripe, fused shapes ---------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("cell", [9232, 50192])
@pytest.mark.parametrize("k,m", [(6, 3), (3, 2), (10, 4), (2, 1)])
def test_short_last_stripe_fused_shapes(dev, k, m, cell, ctype):
    """gf_crc_rows<RowsEncode> behind the full stripes' launch: every length."""
    S = 3
    cod = coder(k, m)
    full = k * cell
    lengths = [dl for dl in data_len_cases(k, cell, S)] + [(S - 1) * full + r for r in cut_lengths(k, cell, tile_of(k))]
    lengths = list(dict.fromkeys(lengths))
    assert len(lengths) >= 10
    cases = []
    for data_len in lengths:
        c = Enc(cod, k, m, cell, last_short(k, cell, S, data_len), dev, ctype=ctype)
        assert c.data_len() == (0 if data_len in (0, S * full) else data_len)
        c.uniform(data_len=data_len)
        cases.append(c)
    torch.cuda.synchronize()
    for c in cases:
        c.check(c.rs[-1])


# ---- 2. the byte-wise route ---------------------------------------------------------

@pytest.mark.parametrize("shape", ["rs42", "bpc1024", "bpc100", "base1", "cell528", "cell1000", "rs65"])
def test_bytewise_route(dev, shape):
    """The shapes the one-pass kernel does not take run gf_encode_rows_bytes
    behind the full stripes' composition: same images."""
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
    S, full = 3, k * cell
    cod = coder(k, m)
    cu = max(1, k // 2)
    lengths = data_len_cases(k, cell, S) + [(S - 1) * full + r
                                            for r in (cu * cell + 1, cu * cell + 17, cu * cell + cell - 1, 77, cell)]
    cases = []
    for li, data_len in enumerate(dict.fromkeys(lengths)):
        c = Enc(cod, k, m, cell, last_short(k, cell, S, data_len), dev, pad=7, ctype=(C32C, C32)[li % 2], **kw)
        c.uniform(data_len=data_len)
        cases.append(c)
    if shape == "base1":
        assert cases[0].cells.data_ptr() % 16 == 1
    torch.cuda.synchronize()
    for c in cases:
        c.check((shape, c.rs[-1]))


# ---- 3. one length per stripe -------------------------------------------------------

def mixed_lengths(k, cell, S=24):
    cycle = [0, k * cell, 1, cell, cell + 1] + cut_lengths(k, cell, tile_of(k))
    return [cycle[(7 * s + 3) % len(cycle)] for s in range(S)]


@pytest.mark.parametrize("route", ["fused", "bytes"])
@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_lengths(dev, k, m, route):
    """24 stripes, per-stripe lengths, one launch over all of them; the
    workspace of exactly the advertised size keeps its guard bands.  Then the
    tensor helper on the same batch."""
    cell = 9232 if route == "fused" else 1000
    bpc = 512 if route == "fused" else 100
    rs = mixed_lengths(k, cell)
    assert any(r == 0 for r in rs) and any(r == k * cell for r in rs)
    S, full = len(rs), k * cell
    true_rs = [r or full for r in rs]
    cod = coder(k, m)
    nbytes = cod.encode_crc_rows_mixed_workspace_size(S)
    assert nbytes == 8 * S
    buf = torch.full((nbytes + 512,), GUARD, dtype=torch.uint8, device=dev)
    ws = buf[256:256 + nbytes]
    assert ws.data_ptr() % 8 == 0
    a = Enc(cod, k, m, cell, true_rs, dev, pad=16, bpc=bpc)
    a.mixed(stripe_bytes=rs, workspace=ws)
    b = Enc(cod, k, m, cell, true_rs, dev, bpc=bpc, ctype=C32)
    b.mixed(stripe_bytes=rs)
    h = Enc(cod, k, m, cell, true_rs, dev, pad=0, bpc=bpc)
    got = H.encode_crc_rows_batch(cod, h.cells, h.sums, stripe_bytes=rs, bytes_per_checksum=bpc)
    assert got.numel() == nbytes
    torch.cuda.synchronize()
    a.check("guarded workspace")
    b.check("crc32")
    h.check("helper")
    assert bool((buf[:256] == GUARD).all()) and bool((buf[256 + nbytes:] == GUARD).all())
    lens = np.frombuffer(ws.cpu().numpy().tobytes(), dtype="<u8").tolist()
    assert lens == true_rs


def test_tensor_helper_uniform_form(dev):
    k, m, cell, S = 6, 3, 9232, 3
    cod = coder(k, m)
    data_len = (S - 1) * k * cell + 3 * cell + 513
    c = Enc(cod, k, m, cell, last_short(k, cell, S, data_len), dev, pad=0)
    assert H.encode_crc_rows_batch(cod, c.cells, c.sums, data_len=data_len) is None
    torch.cuda.synchronize()
    c.check()


# ---- 4. identity with the full-stripe calls -----------------------------------------

@pytest.mark.parametrize("cell", [9232, 1000])
def test_full_stripes_identical_to_encode_crc(dev, cell):
    """data_len == 0 and stripe_bytes NULL / all zero / all k*cell_len /
    alternating: parity and sums byte-identical to hec_encode_crc_device; CRC32
    on full stripes equals hec_encode_device + hec_checksum_device."""
    k, m, S = 6, 3, 9
    cod = coder(k, m)
    full = k * cell
    rs = [full] * S
    ref = Enc(cod, k, m, cell, rs, dev)
    dp, ds, pp, ps = ref.ptr_args()
    cod.encode_crc_device(dp, ds, pp, ps, cell, S, 512, ref.sums.data_ptr(), stream())
    got = [Enc(cod, k, m, cell, rs, dev)]
    got[0].uniform(data_len=0)
    got.append(Enc(cod, k, m, cell, rs, dev))
    got[1].uniform(data_len=S * full)
    for sb in (None, [0] * S, [full] * S, [0, full] * (S // 2) + [0]):
        g = Enc(cod, k, m, cell, rs, dev)
        gdp, gds, gpp, gps = g.ptr_args()
        # no entry is short: no workspace is needed
        cod.encode_crc_rows_device_mixed(gdp, gds, gpp, gps, sb, cell, S, g.sums.data_ptr(), None, 0, stream=stream())
        got.append(g)
    # CRC32
    ref32 = Enc(cod, k, m, cell, rs, dev, ctype=C32)
    dp, ds, pp, ps = ref32.ptr_args()
    cod.encode_device(dp, ds, pp, ps, cell, S, stream())
    cod.checksum_device(C32, dp + pp, ds + ps, cell, S, 512, ref32.sums.data_ptr(), stream())
    got32 = Enc(cod, k, m, cell, rs, dev, ctype=C32)
    got32.uniform(data_len=0)
    mix32 = Enc(cod, k, m, cell, rs, dev, ctype=C32)
    mix32.mixed(stripe_bytes=[0] * S)
    torch.cuda.synchronize()
    ref.check("hec_encode_crc_device")
    for i, g in enumerate(got):
        assert torch.equal(ref.cells, g.cells), i
        assert torch.equal(ref.sums, g.sums), i
    for i, g in enumerate((got32, mix32)):
        assert torch.equal(ref32.cells, g.cells), i
        assert torch.equal(ref32.sums, g.sums), i
        g.check(("crc32", i))


# ---- 5. full stripes through the rows kernel ----------------------------------------

@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_full_stripes_through_the_rows_kernel(dev, k, m):
    """One short stripe among 8 full ones, mixed form: all nine stripes run
    gf_crc_rows<RowsEncode>, and the full ones' parity and sums are the oracle's."""
    cell = 9232
    full = k * cell
    rs = [full] * 9
    rs[4] = 3 * cell + 513
    cod = coder(k, m)
    sb = [0 if (r == full and s % 2) else r for s, r in enumerate(rs)]
    runs = [Enc(cod, k, m, cell, rs, dev, ctype=ct) for ct in (C32C, C32)]
    for c in runs:
        c.mixed(stripe_bytes=sb)
    torch.cuda.synchronize()
    for c in runs:
        c.check(c.ctype)
        for s in range(9):
            if s != 4:
                assert bool((c.sums[s] != SENT).any(dim=-1).all()), s  # every slot of a full stripe is live


# ---- 6. a file-order buffer ---------------------------------------------------------

@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (4, 2, 1000)])
def test_file_order_buffer(dev, k, m, cell):
    """One contiguous [rows][k][cell] allocation holds data_len file bytes
    followed by 0xEE: usable as it is.  Parity [0, n0) equals what
    hec_encode_rows_device writes for the same file, and both the oracle's."""
    rows, full = 3, k * cell
    cod = coder(k, m)
    runs = []
    for r in (777, cell + 17, 3 * cell + 513, full - 1):
        data_len = (rows - 1) * full + r
        rs = last_short(k, cell, rows, data_len)
        t, lens = stripes_truth("rs", k, m, cell, rs)
        true = stripes_sums("rs", k, m, cell, rs, 512, C32C)
        file_host = np.full((rows * full,), GARBAGE, dtype=np.uint8)
        file_host[:data_len] = np.ascontiguousarray(t[:, :k]).reshape(-1)[:data_len]
        d = torch.from_numpy(file_host).to(dev)
        par = torch.full((rows, m, cell), OUTFILL, dtype=torch.uint8, device=dev)
        sums = torch.full((rows, k + m, -(-cell // 512), 4), SENT, dtype=torch.uint8, device=dev)
        cod.encode_crc_rows_device([d.data_ptr() + i * cell for i in range(k)], [full] * k,
                                   [par.data_ptr() + j * cell for j in range(m)], [m * cell] * m, cell, rows,
                                   sums.data_ptr(), data_len=data_len, stream=stream())
        par2 = torch.full((rows, m, cell), OUTFILL, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(16, cod.encode_rows_workspace_size(cell)), dtype=torch.uint8, device=dev)
        cod.encode_rows_device(d.data_ptr(), data_len, par2.data_ptr(), cell, ws.data_ptr(), ws.numel(), stream())
        runs.append((r, t, true, file_host, d, par, par2, sums, ws))
    torch.cuda.synchronize()
    for r, t, true, file_host, d, par, par2, sums, ws in runs:
        n0 = min(cell, r)
        want = np.full((rows, m, cell), OUTFILL, dtype=np.uint8)
        want[:rows - 1] = t[:rows - 1, k:]
        want[rows - 1, :, :n0] = t[rows - 1, k:, :n0]
        assert np.array_equal(par.cpu().numpy(), want), r
        assert torch.equal(par[:rows - 1], par2[:rows - 1]) and torch.equal(par[rows - 1, :, :n0], par2[rows - 1, :, :n0]), r
        assert np.array_equal(sums.cpu().numpy(), true), r
        assert np.array_equal(d.cpu().numpy(), file_host), r


# ---- 7. codecs ----------------------------------------------------------------------

@pytest.mark.parametrize("codec,k,m,cell,bpc", [("rs-legacy", 6, 3, 9232, 512), ("xor", 2, 1, 9232, 512),
                                                 ("xor", 2, 1, 1000, 100)])
def test_codecs(dev, codec, k, m, cell, bpc):
    S = 3
    cod = coder(k, m, codec)
    r = max(1, k // 2) * cell + 513 if cell > 1000 else cell + 317
    rs = [k * cell] * (S - 1) + [r]
    runs = [Enc(cod, k, m, cell, rs, dev, codec=codec, bpc=bpc, ctype=ct) for ct in (C32C, C32)]
    runs[0].uniform()
    runs[1].mixed()
    torch.cuda.synchronize()
    for c in runs:
        c.check((codec, c.ctype))


# ---- 8. write -> scrub -> composite -------------------------------------------------

@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (10, 4, 9232), (4, 2, 1000)])
def test_write_scrub_composite(dev, k, m, cell, ctype):
    """encode_crc_rows_device, scrub_crc_rows_device with d_expected = the sums
    just written, composite_crc_device, one stream and one sums array."""
    n, S, bpc = k + m, 3, 512
    cod = coder(k, m)
    runs = []
    for data_len in data_len_cases(k, cell, S):
        c = Enc(cod, k, m, cell, last_short(k, cell, S, data_len), dev, ctype=ctype)
        c.uniform(data_len=data_len)
        ptrs, strides = slots(c.cells)
        res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
        bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        cod.scrub_crc_rows_device(ptrs, strides, cell, S, c.sums.data_ptr(), bad.data_ptr(), res.data_ptr(),
                                  data_len=data_len, stream=stream(), **c.kw())
        _, unit, grp = H.composite_crc_batch(cod, c.sums, k, cell, ctype, bpc, data_len, want=("unit", "group"))
        runs.append((c, data_len, res, bad, unit, grp))
    # the mixed-form twin: every stripe its own length
    rs = [3 * cell + 513 if k > 4 else cell + 317, k * cell, 777]
    c = Enc(cod, k, m, cell, rs, dev, ctype=ctype)
    c.mixed()
    ptrs, strides = slots(c.cells)
    res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
    bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
    sws = torch.empty(cod.scrub_crc_rows_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    cod.scrub_crc_rows_device_mixed(ptrs, strides, [(1 << n) - 1] * S, rs, cell, S, c.sums.data_ptr(), bad.data_ptr(),
                                    res.data_ptr(), sws.data_ptr(), sws.numel(), stream=stream(), **c.kw())
    torch.cuda.synchronize()
    c.check("mixed")
    assert res.tolist() == [[0, 0]] * S and not bool(bad.any())
    for c, data_len, res, bad, unit, grp in runs:
        c.check(data_len)
        assert res.tolist() == [[0, 0]] * S, (data_len, res.tolist())
        assert not bool(bad.any()), data_len
        units, group = c.crcs(data_len)
        assert be32(unit) == units, data_len
        assert be32(grp)[0] == group, data_len


# ---- 9. write -> lose -> repair -----------------------------------------------------

def test_write_lose_repair(dev):
    """After the encode, units (1, k) are overwritten with garbage and their
    sums with the sentinel; the rows repair in place with d_expected == d_sums
    brings back the cells' [0, len) and the live sums, no flag set."""
    k, m, cell, S = 6, 3, 9232, 3
    n, full = k + m, k * cell
    cod = coder(k, m)
    runs = []
    for r in (777, cell + 17, 3 * cell + 513):
        c = Enc(cod, k, m, cell, [full] * (S - 1) + [r], dev)
        c.uniform()
        lost = (1, k)
        for u in lost:
            c.cells[:, u] = 0x5C
            c.sums[:, u] = SENT
        ptrs, strides = slots(c.cells)
        shards = [None if i in lost else ptrs[i] for i in range(n)]
        bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        cod.reconstruct_crc_rows_device(shards, strides, ptrs, strides, cell, S, c.sums.data_ptr(),
                                        data_len=c.data_len(), expected_ptr=c.sums.data_ptr(), bad_ptr=bad.data_ptr(),
                                        stream=stream())
        runs.append((c, bad))
    torch.cuda.synchronize()
    for c, bad in runs:
        assert not bool(bad.any()), c.rs[-1]
        assert torch.equal(c.sums, c.exp_sums), c.rs[-1]
        for s in range(S):
            for u in range(n):
                ln = c.lens[s][u]
                assert torch.equal(c.cells[s, u, :ln], c.exp_cells[s, u, :ln]), (c.rs[-1], s, u)


# ---- 10. graph ----------------------------------------------------------------------

def test_graph_capture_replay_with_composite(dev):
    """The uniform form and hec_composite_crc_device captured on a side stream
    and replayed twice on fresh sentinel-filled outputs."""
    k, m, n, S, cell, bpc = 6, 3, 9, 3, 9232, 512
    data_len = (S - 1) * k * cell + 3 * cell + 513
    cod = coder(k, m)
    c = Enc(cod, k, m, cell, last_short(k, cell, S, data_len), dev)
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
    units, group = c.crcs(data_len)
    for rep in range(2):
        c.reset()
        unit.fill_(SENT)
        grp.fill_(SENT)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.check(("replay", rep))
        assert be32(unit) == units, rep
        assert be32(grp)[0] == group, rep


# ---- 11. argument errors on the device, nothing queued -------------------------------

def test_argument_errors_write_nothing(dev):
    k, m, S, cell = 6, 3, 4, 9232
    cod = coder(k, m)
    full = k * cell
    rs = [full] * (S - 1) + [cell + 5]
    c = Enc(cod, k, m, cell, rs, dev)
    dp, ds, pp, ps = c.ptr_args()
    nbytes = cod.encode_crc_rows_mixed_workspace_size(S)
    buf = torch.full((nbytes + 16 + 512,), GUARD, dtype=torch.uint8, device=dev)
    wp, wn = buf[256:].data_ptr(), nbytes + 16
    sp = c.sums.data_ptr()

    def uniform(data=dp, parity=pp, sums_ptr=sp, stripes=S, data_len=c.data_len(), **kw):
        with pytest.raises(ValueError):
            cod.encode_crc_rows_device(data, ds, parity, ps, cell, stripes, sums_ptr, data_len=data_len,
                                       stream=stream(), **kw)

    def mixed(data=dp, parity=pp, sums_ptr=sp, lens=rs, ws=wp, ws_bytes=wn, **kw):
        with pytest.raises(ValueError):
            cod.encode_crc_rows_device_mixed(data, ds, parity, ps, lens, cell, S, sums_ptr, ws, ws_bytes,
                                             stream=stream(), **kw)

    for call in (uniform, mixed):
        call(checksum_type=H.CHECKSUM_NULL)
        call(checksum_type=7)
        call(bytes_per_checksum=0)
        call(sums_ptr=None)
        call(sums_ptr=sp + 2)
        call(parity=[pp[0], None, pp[2]])
        call(data=[None] + dp[1:])
        call(data=None)
        call(parity=None)
    for S_, data_len in ((S, (S - 1) * full), (S, 1), (S, S * full + 1), (0, 5)):
        uniform(stripes=S_, data_len=data_len)
    mixed(lens=[full + 1] + rs[1:])
    mixed(lens=[2 ** 63] + rs[1:])
    # a stripe is short: the workspace NULL, one byte short, misaligned
    mixed(ws=None)
    mixed(ws_bytes=nbytes - 1)
    mixed(ws=wp + 4)
    torch.cuda.synchronize()
    c.no_change("errors")
    assert bool((buf == GUARD).all())
    # no stripes: OK, and still nothing written
    cod.encode_crc_rows_device(dp, ds, pp, ps, cell, 0, sp, stream=stream())
    cod.encode_crc_rows_device_mixed(dp, ds, pp, ps, [], cell, 0, sp, None, 0, stream=stream())
    torch.cuda.synchronize()
    c.no_change("no stripes")
    # no stripe is short: a NULL workspace is accepted
    f = Enc(cod, k, m, cell, [full] * S, dev)
    fdp, fds, fpp, fps = f.ptr_args()
    cod.encode_crc_rows_device_mixed(fdp, fds, fpp, fps, [0, full, 0, full], cell, S, f.sums.data_ptr(), None, 0,
                                     stream=stream())
    torch.cuda.synchronize()
    f.check("full, no workspace")
    assert bool((buf == GUARD).all())
