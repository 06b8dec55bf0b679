"""Composite CRCs on the device (hec_composite_crc_device).  Every call is
checked exactly, whole arrays, against (a) the oracle's CRC over the actual
concatenated bytes or (b) composite_crc_ref.py, never against the code under
test; the host call on the same sums must agree as well.

The shapes are the smallest that cross every boundary of the kernels: a
sub-wave per cell (nck - 1 < 64), one lane per chunk (nck = 65), more than one
chunk per lane (nck = 99, 128), lane groups that are not full, more than one
1024-cell block of partials per fold (257 stripes of 32 data units, 4099
stripes) and 64-bit exponents (bpc = cell = 2^30)."""
import ctypes
import functools

import numpy as np
import pytest

import composite_crc_cases as cases
import composite_crc_ref as ref
import ec_oracle
import hdfs_native_ec as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TYPES = (H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32)
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_coders = {}


def coder(k=6, m=3):
    if (k, m) not in _coders:
        _coders[(k, m)] = H.Coder(k, m, 0)
    return _coders[(k, m)]


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def truth(ctype, n, k, cell, stripes, bpc, data_len):
    """Computed once per case and shared: (sums, cells, units, group)."""
    out = cases.build(ec_oracle.load_c_oracle(), ctype, n, k, cell, stripes, bpc, data_len,
                      seed=hash((n, k, cell, stripes, bpc, data_len)) & 0xFFFFFF)
    for a in out[:3]:
        a.setflags(write=False)
    return out


class Banded:
    """`size` bytes of device memory between two 0xA5 guard bands."""

    def __init__(self, size, dev):
        self.size = size
        self.buf = torch.full((size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)

    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def guards_intact(self):
        raw = self.buf.cpu().numpy()
        return bool((raw[:GUARD] == 0xA5).all() and (raw[GUARD + self.size:] == 0xA5).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all())

    def words(self):
        return cases.be_words(self.buf.cpu().numpy()[GUARD:GUARD + self.size].tobytes())


class Call:
    """One hec_composite_crc_device call: outputs and an exact-size workspace
    inside guard bands, the sums on the device."""

    def __init__(self, dev, sums, n, want=(True, True, True)):
        self.sums_host = np.ascontiguousarray(sums)
        self.stripes = sums.shape[0]
        self.n = n
        self.want = want
        self.d_sums = torch.from_numpy(self.sums_host.copy()).to(dev)
        self.out = [Banded(size, dev) for size in (4 * self.stripes * n, 4 * n, 4)]
        self.ws = Banded(H.composite_crc_workspace_size(n, self.stripes), dev)

    def launch(self, ctype, k, cell, bpc, data_len, strm=None, cod=None):
        ptrs = [o.ptr() if w else 0 for o, w in zip(self.out, self.want)]
        (cod or coder()).composite_crc_device(ctype, self.d_sums.data_ptr(), self.n, k, cell, self.stripes, bpc,
                                              data_len, ptrs[0], ptrs[1], ptrs[2], self.ws.ptr(), self.ws.size,
                                              stream() if strm is None else strm)

    def results(self):
        """After a synchronise: hygiene, then (cells, units, group) as uint32
        arrays, None for an output that was passed as NULL."""
        assert np.array_equal(self.d_sums.cpu().numpy(), self.sums_host), "d_sums was written"
        assert self.ws.guards_intact(), "workspace guard bands"
        got = []
        for o, w in zip(self.out, self.want):
            assert o.guards_intact(), "output guard bands"
            if not w:
                assert o.untouched(), "a NULL output was written"
            got.append(o.words() if w else None)
        return got


def host_result(ctype, sums, n, k, cell, stripes, bpc, data_len):
    cells, units, group = H.composite_crc(ctype, np.ascontiguousarray(sums).tobytes(), n, k, cell, stripes, bpc,
                                          data_len)
    return np.array(cells, dtype=np.uint32).reshape(-1), np.array(units, dtype=np.uint32), group


def check_case(dev, ctype, n, k, cell, stripes, bpc, data_len):
    sums, cells, units, group = truth(ctype, n, k, cell, stripes, bpc, data_len)
    calls = [Call(dev, sums, n, want) for want in
             ((True, True, True), (True, False, False), (False, True, False), (False, False, True))]
    for c in calls:
        c.launch(ctype, k, cell, bpc, data_len)
    torch.cuda.synchronize()
    got = [c.results() for c in calls]
    where = (ctype, n, k, cell, stripes, bpc, data_len)
    assert np.array_equal(got[0][0], cells.reshape(-1)), where
    assert np.array_equal(got[0][1], units), where
    assert got[0][2][0] == group, where
    # each single-output call equals the all-outputs call
    assert np.array_equal(got[1][0], got[0][0]), where
    assert np.array_equal(got[2][1], got[0][1]), where
    assert np.array_equal(got[3][2], got[0][2]), where
    # and the host call on the same sums
    h = host_result(ctype, sums, n, k, cell, stripes, bpc, data_len)
    assert np.array_equal(h[0], got[0][0]) and np.array_equal(h[1], got[0][1]) and h[2] == got[0][2][0], where


NK = ((9, 6), (14, 10), (5, 3), (1, 1), (64, 32))

# chunks per cell at 512-byte chunks: 1, 2 with a short tail, 19, 99, 64, 65, 128
CHUNK_SHAPES = [(cell, 512, stripes, NK[i % 5], i % 5)
                for i, (cell, stripes) in enumerate(((16, 3), (528, 2), (9232, 3), (50192, 1), (32768, 2), (33280, 2),
                                                     (65536, 1), (528, 1), (9232, 2), (33280, 1)))]
# other chunk sizes
CHUNK_SHAPES += [(1000, 256, 3, (9, 6), 4), (37, 256, 2, (14, 10), 3), (1000, 4096, 2, (5, 3), 2),
                 (37, 4096, 3, (64, 32), 1), (1000, 256, 1, (1, 1), 0)]


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("cell,bpc,stripes,nk,dl", CHUNK_SHAPES)
def test_chunk_shapes(dev, ctype, cell, bpc, stripes, nk, dl):
    n, k = nk
    check_case(dev, ctype, n, k, cell, stripes, bpc, cases.data_len_cases(k, cell, stripes)[dl])


# many stripes, 16-byte cells: the folds over cells, up to several blocks of partials
STRIPE_SHAPES = [(64, (9, 6), 2), (65, (14, 10), 3), (65, (1, 1), 0), (257, (64, 32), 4), (257, (5, 3), 1),
                 (4099, (5, 3), 3), (4099, (9, 6), 2)]


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("stripes,nk,dl", STRIPE_SHAPES)
def test_stripe_counts(dev, ctype, stripes, nk, dl):
    n, k = nk
    check_case(dev, ctype, n, k, 16, stripes, 512, cases.data_len_cases(k, 16, stripes)[dl])


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("geom", ((9, 6, 9232, 3, 512), (14, 10, 528, 2, 512), (5, 3, 33280, 2, 512), (1, 1, 1000, 3, 256)))
def test_every_data_len_case(dev, ctype, geom):
    n, k, cell, stripes, bpc = geom
    for data_len in cases.data_len_cases(k, cell, stripes):
        check_case(dev, ctype, n, k, cell, stripes, bpc, data_len)


def opaque_sums(n, k, cell, stripes, bpc, data_len, seed, dead, parity_fill=None):
    rng = np.random.default_rng(seed)
    nck = -(-cell // bpc)
    sums = rng.integers(0, 256, (stripes, n, nck, 4), dtype=np.uint8)
    lens = ref.cell_lengths(n, k, cell, stripes, data_len)
    for u in range(n):
        sums[stripes - 1, u, -(-lens[stripes - 1][u] // bpc):] = dead
    if parity_fill is not None:
        sums[:, k:] = parity_fill
    return sums


@pytest.mark.parametrize("ctype", TYPES)
@pytest.mark.parametrize("geom", ((9, 6, 2**30, 8, 2**30, 0), (9, 6, 2**30, 8, 2**30, 7 * 6 * 2**30 + 2**30 + 5),
                                  (5, 3, 1000, 3, 256, 2 * 3 * 1000 + 1000 + 300),
                                  (14, 10, 50192, 2, 512, 10 * 50192 + 3 * 50192 + 700)))
def test_opaque_sums_against_definition(dev, ctype, geom):
    """Sums that are the CRC of no data, unit lengths past 2^32; the slots no
    chunk covers and the parity slots do not reach the outputs they must not."""
    n, k, cell, stripes, bpc, data_len = geom
    variants = [opaque_sums(n, k, cell, stripes, bpc, data_len, 11, 0xA5), opaque_sums(n, k, cell, stripes, bpc, data_len, 11, 0x5A),
                opaque_sums(n, k, cell, stripes, bpc, data_len, 11, 0xA5, 0xA5),
                opaque_sums(n, k, cell, stripes, bpc, data_len, 11, 0x5A, 0x5A)]
    ints = variants[0].view(">u4")[..., 0].astype(np.uint32).tolist()
    want_cells, want_units, want_group = ref.composite(ctype, ints, n, k, cell, stripes, bpc, data_len)
    calls = [Call(dev, v, n) for v in variants]
    for c in calls:
        c.launch(ctype, k, cell, bpc, data_len)
    torch.cuda.synchronize()
    got = [c.results() for c in calls]
    assert got[0][0].reshape(stripes, n).tolist() == want_cells
    assert got[0][1].tolist() == want_units
    assert got[0][2][0] == want_group
    for x, y in zip(got[0], got[1]):
        assert np.array_equal(x, y)
    for g in got[2:]:
        assert g[2][0] == want_group
        assert g[1][:k].tolist() == want_units[:k]
        assert g[0].reshape(stripes, n)[:, :k].tolist() == [row[:k] for row in want_cells]
    for v, g in zip(variants, got):
        h = host_result(ctype, v, n, k, cell, stripes, bpc, data_len)
        assert np.array_equal(h[0], g[0]) and np.array_equal(h[1], g[1]) and h[2] == g[2][0]


def test_invalid_arguments_queue_nothing(dev):
    n, k, cell, stripes, bpc = 9, 6, 528, 3, 512
    sums = truth(H.CHECKSUM_CRC32C, n, k, cell, stripes, bpc, 0)[0]
    c = Call(dev, sums, n)
    cod = coder()
    ok = dict(h=cod.handle, ctype=H.CHECKSUM_CRC32C, sums=c.d_sums.data_ptr(), n=n, k=k, cell=cell, stripes=stripes,
              bpc=bpc, data_len=0, cells=c.out[0].ptr(), units=c.out[1].ptr(), group=c.out[2].ptr(), ws=c.ws.ptr(),
              ws_bytes=c.ws.size)

    def call(**kw):
        a = dict(ok, **kw)
        vp = ctypes.c_void_p
        return H.lib.hec_composite_crc_device(a["h"], a["ctype"], vp(a["sums"]), a["n"], a["k"], a["cell"],
                                              a["stripes"], a["bpc"], a["data_len"], vp(a["cells"]), vp(a["units"]),
                                              vp(a["group"]), vp(a["ws"]), a["ws_bytes"], vp(stream()))

    full = stripes * k * cell
    refused = [dict(h=None), dict(sums=None), dict(sums=ok["sums"] + 2), dict(cells=ok["cells"] + 1),
               dict(units=ok["units"] + 2), dict(group=ok["group"] + 3), dict(cell=0), dict(bpc=0), dict(n=0),
               dict(n=65), dict(k=0), dict(k=n + 1), dict(data_len=full + 1), dict(data_len=full - k * cell),
               dict(ctype=H.CHECKSUM_NULL), dict(ctype=3), dict(ws=None), dict(ws=ok["ws"] + 2),
               dict(ws_bytes=c.ws.size - 1), dict(ws=None, cells=None, units=None),
               dict(ws_bytes=0, cells=None, group=None)]
    for bad in refused:
        assert call(**bad) == H.HEC_ERR_INVALID_ARG, bad
    # nothing to do: no stripes, no output; cells alone need no workspace
    assert call(stripes=0) == H.HEC_OK
    assert call(cells=None, units=None, group=None, ws=None, ws_bytes=0) == H.HEC_OK
    torch.cuda.synchronize()
    assert all(o.untouched() for o in c.out) and c.ws.untouched()
    assert call(units=None, group=None, ws=None, ws_bytes=0) == H.HEC_OK
    torch.cuda.synchronize()
    assert c.ws.untouched() and c.out[1].untouched() and c.out[2].untouched()
    assert np.array_equal(c.out[0].words(), truth(H.CHECKSUM_CRC32C, n, k, cell, stripes, bpc, 0)[1].reshape(-1))


# ---- end to end on one stream, nothing synchronised in between ----------------

def oracle_units(ctype, cells_np):
    """CRC of every cell, every unit and the data of a numpy [S, n, cell] image."""
    clib = ec_oracle.load_c_oracle()
    S, n, _ = cells_np.shape
    cell_crcs = np.array([[cases.oracle_crc(clib, ctype, cells_np[s, u]) for u in range(n)] for s in range(S)],
                         dtype=np.uint32)
    unit_crcs = np.array([cases.oracle_crc(clib, ctype, cells_np[:, u].reshape(-1)) for u in range(n)], dtype=np.uint32)
    return cell_crcs, unit_crcs


@pytest.mark.parametrize("k,m", ((6, 3), (10, 4), (3, 2)))
def test_encode_crc_then_composite(dev, k, m):
    S, cell, n = 5, 9216, k + m
    rng = np.random.default_rng(100 * k + m)
    cells = torch.from_numpy(rng.integers(0, 256, (S, n, cell), dtype=np.uint8)).to(dev)
    sums = torch.zeros((S, n, cell // 512, 4), dtype=torch.uint8, device=dev)
    ptrs, strides = H.stripe_layout_ptrs(cells, n)
    cod = coder(k, m)
    cod.encode_crc_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], cell, S, 512, sums.data_ptr(), stream())
    got = H.composite_crc_batch(cod, sums, k, cell)
    torch.cuda.synchronize()
    image = cells.cpu().numpy()
    clib = ec_oracle.load_c_oracle()
    for s in range(S):  # the parity the CRCs are taken over is the oracle's
        want = ec_oracle.c_encode(clib, k, m, list(image[s, :k]))
        for j in range(m):
            assert np.array_equal(image[s, k + j], want[j])
    cell_crcs, unit_crcs = oracle_units(H.CHECKSUM_CRC32C, image)
    assert np.array_equal(cases.be_words(got[0].cpu().numpy().tobytes()), cell_crcs.reshape(-1))
    assert np.array_equal(cases.be_words(got[1].cpu().numpy().tobytes()), unit_crcs)
    group = cases.oracle_crc(clib, H.CHECKSUM_CRC32C, np.ascontiguousarray(image[:, :k]).reshape(-1))
    assert cases.be_words(got[2].cpu().numpy().tobytes())[0] == group


@pytest.mark.parametrize("ctype", TYPES)
def test_reconstruct_crc_then_composite(dev, ctype):
    """A lost unit's cells and sum slots are refilled by the verified
    reconstruction (d_expected == d_sums); the composite call behind it on
    the same stream reports the original units' CRCs."""
    k, m, S, cell, lost = 6, 3, 4, 9216, 4
    n = k + m
    rng = np.random.default_rng(77 + ctype)
    data = rng.integers(0, 256, (S, k, cell), dtype=np.uint8)
    clib = ec_oracle.load_c_oracle()
    image = np.zeros((S, n, cell), dtype=np.uint8)
    for s in range(S):
        image[s, :k] = data[s]
        image[s, k:] = np.stack(ec_oracle.c_encode(clib, k, m, list(data[s])))
    true_sums = np.zeros((S, n, cell // 512, 4), dtype=np.uint8)
    for s in range(S):
        for u in range(n):
            clib.orc_chunk_checksum(ctype, image[s, u].ctypes.data_as(ctypes.c_void_p), cell, 512,
                                    true_sums[s, u].ctypes.data_as(ctypes.c_void_p))
    broken, broken_sums = image.copy(), true_sums.copy()
    broken[:, lost] = 0xEE
    broken_sums[:, lost] = 0xEE
    cells = torch.from_numpy(broken).to(dev)
    sums = torch.from_numpy(broken_sums).to(dev)
    bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
    ptrs, strides = H.stripe_layout_ptrs(cells, n)
    cod = coder(k, m)
    cod.reconstruct_crc_device([None if i == lost else ptrs[i] for i in range(n)], strides, ptrs, strides, cell, S,
                               sums.data_ptr(), expected_ptr=sums.data_ptr(), bad_ptr=bad.data_ptr(),
                               checksum_type=ctype, stream=stream())
    got = H.composite_crc_batch(cod, sums, k, cell, checksum_type=ctype)
    torch.cuda.synchronize()
    assert not bool(bad.any())
    assert np.array_equal(cells.cpu().numpy(), image)
    cell_crcs, unit_crcs = oracle_units(ctype, image)
    assert np.array_equal(cases.be_words(got[1].cpu().numpy().tobytes()), unit_crcs)
    assert np.array_equal(cases.be_words(got[0].cpu().numpy().tobytes()), cell_crcs.reshape(-1))


# ---- ordering ------------------------------------------------------------------

def test_graph_capture_and_replay(dev):
    ctype, n, k, cell, stripes, bpc = H.CHECKSUM_CRC32C, 9, 6, 9232, 3, 512
    first = truth(ctype, n, k, cell, stripes, bpc, 0)
    other = cases.build(ec_oracle.load_c_oracle(), ctype, n, k, cell, stripes, bpc, 0, seed=4242)
    assert not np.array_equal(first[0], other[0])
    c = Call(dev, first[0], n)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c.launch(ctype, k, cell, bpc, 0, strm=side.cuda_stream)  # warm: nothing in the capture is a first use
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        c.launch(ctype, k, cell, bpc, 0, strm=torch.cuda.current_stream().cuda_stream)
    for want in (first, other):
        c.sums_host = np.ascontiguousarray(want[0])
        c.d_sums.copy_(torch.from_numpy(c.sums_host.copy()))
        for o in c.out:
            o.buf.fill_(0xA5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = c.results()
        assert np.array_equal(got[0], want[1].reshape(-1))
        assert np.array_equal(got[1], want[2])
        assert got[2][0] == want[3]


def test_two_streams_with_separate_workspaces(dev):
    ctype, n, k, bpc = H.CHECKSUM_CRC32, 14, 10, 512
    a = truth(ctype, n, k, 16, 4099 // 2, bpc, 0)
    b = truth(ctype, n, k, 9232, 3, bpc, cases.data_len_cases(k, 9232, 3)[4])
    ca, cb = Call(dev, a[0], n), Call(dev, b[0], n)
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for _ in range(2):
        ca.launch(ctype, k, 16, bpc, 0, strm=sa.cuda_stream)
        cb.launch(ctype, k, 9232, bpc, cases.data_len_cases(k, 9232, 3)[4], strm=sb.cuda_stream)
    torch.cuda.synchronize()
    for c, want in ((ca, a), (cb, b)):
        got = c.results()
        assert np.array_equal(got[0], want[1].reshape(-1))
        assert np.array_equal(got[1], want[2])
        assert got[2][0] == want[3]
