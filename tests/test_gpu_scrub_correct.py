"""Scrub correction on the GPU (hec_scrub_correct_device: the gf_scrub_correct
register kernel and the byte-granular gf_scrub_correct_bytes).  Expected
values come from scrub_correct_ref.py, a numpy restatement of the definition
over the oracle's matrix and product table: the verdict from the reference
pair, then e = scale * s_row applied to the named unit, so every case --
the m == 2 stripes with two corrupt units too -- has a defined outcome.  Every
comparison is exact and whole: the cells tensor with a guard stripe of 0xA5 on
either side, and the units array, handed in filled with 0x7F7F7F7F (the call
writes every entry itself).  The results the correction reads come from
scrub_batch on the same stream."""
import ctypes

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
import scrub_correct_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S = 37  # as test_gpu_scrub.py
TILE = {2: 4096, 3: 4096, 6: 4096, 10: 2048}  # bytes of a wave-tile of the register kernel, by k
FILL = 0x7F7F7F7F
GUARD = 0xA5

# (codec, k, m, cell): one wave-tile + 16 bytes at all 16 (k, m) of the
# register kernel, M == 1 again with xor, rs-legacy, and (6,3) / (10,4) at one
# chunk and at exactly one wave-tile
REGISTER = [("rs", k, m, TILE[k] + 16) for k in (2, 3, 6, 10) for m in (1, 2, 3, 4)]
REGISTER += [("rs-legacy", k, m, TILE[k] + 16) for k, m in ((3, 2), (6, 3), (10, 4))]
REGISTER += [("xor", k, 1, TILE[k] + 16) for k in (2, 3, 6, 10)]
REGISTER += [("rs", 6, 3, 16), ("rs", 6, 3, 4096), ("rs", 10, 4, 16), ("rs", 10, 4, 2048)]
# the byte kernel: k or m outside the register kernel's, an odd cell length
BYTE = [("rs", 5, 3, 4112), ("xor", 5, 1, 4112), ("rs", 4, 8, 4099), ("rs", 32, 16, 4099), ("rs", 1, 2, 4099),
        ("rs", 6, 3, 4099)]


def ids(cases):
    return [f"{c}-{k}-{m}-{cell}" for c, k, m, cell in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_coders = {}


def coder(k, m, codec="rs"):
    if (k, m, codec) not in _coders:
        _coders[(k, m, codec)] = H.Coder(k, m, 0, codec=codec)
    return _coders[(k, m, codec)]


_truth = {}


def truth(codec, k, m, stripes, cell):
    """Consistent stripes [stripes, k+m, cell], computed once per shape, shared, read-only."""
    key = (codec, k, m, stripes, cell)
    if key not in _truth:
        rng = np.random.default_rng(7919 * k + 37 * m + stripes + cell + len(codec))
        t = np.empty((stripes, k + m, cell), dtype=np.uint8)
        t[:, :k] = rng.integers(0, 256, size=(stripes, k, cell), dtype=np.uint8)
        flat = [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)]
        par = O.matmul_shards(O.codec_matrix(codec, k, m)[k:], flat)
        for j in range(m):
            t[:, k + j] = par[j].reshape(stripes, cell)
        t.setflags(write=False)
        _truth[key] = t
    return _truth[key]


def corrupt(codec, k, m, cell, seed=0):
    """The test image of one shape: six patterns cycled over the stripes --
    clean; one byte at offset 0; the last byte of the cell (with a cell of one
    wave-tile + 16 bytes, the lane past the first wave-tile); the bytes on
    either side of the first chunk boundary and of the boundary into the
    16-byte remainder (15, 16, cell-17, cell-16); a wholly random unit; two
    units.  The single-unit patterns walk through the unit indices, so every
    unit 0..k+m-1 is hit (n <= 24; evenly spread over a wider stripe).
    Returns (cells, single): single maps stripe -> its one corrupt unit."""
    n = k + m
    cells = truth(codec, k, m, S, cell).copy()
    rng = np.random.default_rng(1000 * seed + cell + k)
    locating = [s for s in range(S) if s % 6 in (1, 2, 3, 4)]
    walk = list(range(n)) if n <= len(locating) else [int(v) for v in np.linspace(0, n - 1, len(locating))]
    single = {}
    for x, s in enumerate(locating):
        t = walk[(x + seed) % len(walk)]
        single[s] = t
        if s % 6 == 1:
            cells[s, t, 0] ^= 1 + (x % 255)
        elif s % 6 == 2:
            cells[s, t, cell - 1] ^= 0x80 >> (x % 8)
        elif s % 6 == 3:
            for o in sorted({o for o in (15, 16, cell - 17, cell - 16) if 0 <= o < cell}):
                cells[s, t, o] ^= 0x11 + x
        else:
            cells[s, t] ^= rng.integers(1, 256, size=cell, dtype=np.uint8)  # every byte differs
    for s in range(S):
        if s % 6 == 5 and n >= 2:
            a, b = (s // 6) % n, ((s // 6) * 5 + 1) % n
            if a == b:
                b = (a + 1) % n
            pos = (cell // 2, cell - 1)[(s // 6) % 2]
            cells[s, a, pos] ^= 0x21 + s
            cells[s, b, pos if s % 12 == 5 else 0] ^= 0xC0 - s  # one position, or two
    return cells, single


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(cells, dev):
    """cells [S, n, cell] on the device between two guard stripes: (buf, view)."""
    buf = torch.full((cells.shape[0] + 2,) + cells.shape[1:], GUARD, dtype=torch.uint8, device=dev)
    buf[1:-1] = torch.from_numpy(np.ascontiguousarray(cells)).to(dev)
    return buf, buf[1:-1]


def with_guards(cells):
    out = np.full((cells.shape[0] + 2,) + cells.shape[1:], GUARD, dtype=np.uint8)
    out[1:-1] = cells
    return out


def as_u64(res):
    return res.cpu().numpy().view(np.uint64)


def run_case(codec, k, m, cell, dev, seed=0):
    cells, single = corrupt(codec, k, m, cell, seed)
    want_res, want_units, want_cells = R.correct_batch(codec, k, m, cells)
    cod = coder(k, m, codec)
    buf, view = guarded(cells, dev)
    units = torch.full((S,), FILL, dtype=torch.int32, device=dev)
    res = H.scrub_batch(cod, view)
    got_units = H.scrub_correct_batch(cod, view, res, units)
    torch.cuda.synchronize()
    assert got_units is units
    assert np.array_equal(as_u64(res), want_res)  # the correction read what the reference expects, and left it alone
    assert np.array_equal(units.cpu().numpy(), want_units), (units.cpu().tolist(), want_units.tolist())
    got = buf.cpu().numpy()
    assert np.array_equal(got, with_guards(want_cells)), np.argwhere(got != with_guards(want_cells))[:8].tolist()
    # the closed forms, on the reference itself
    clean = truth(codec, k, m, S, cell)
    for s in range(S):
        if s % 6 == 0:
            assert want_units[s] == R.CLEAN
        elif s in single:
            assert want_units[s] == (single[s] if m > 1 else R.UNLOCATED), s
            if m > 1:
                assert np.array_equal(want_cells[s], clean[s]), s  # one corrupt unit comes back bit-exact
        if want_units[s] < 0:
            assert np.array_equal(want_cells[s], cells[s]), s
        if s % 6 == 5 and m != 2:
            assert want_units[s] == R.UNLOCATED, s
    if m > 1 and k + m <= 24:
        assert set(want_units[want_units >= 0].tolist()) >= set(range(k + m))
    return want_units


@pytest.mark.parametrize("codec,k,m,cell", REGISTER, ids=ids(REGISTER))
def test_register_kernel_equals_reference(dev, codec, k, m, cell):
    assert cell % 16 == 0 and k in TILE and m <= 4
    run_case(codec, k, m, cell, dev)


@pytest.mark.parametrize("codec,k,m,cell", BYTE, ids=ids(BYTE))
def test_byte_kernel_equals_reference(dev, codec, k, m, cell):
    want_units = run_case(codec, k, m, cell, dev)
    if (k, m) == (32, 16):  # units on both sides of bit 32 of the 64-bit word
        located = set(want_units[want_units >= 0].tolist())
        assert {0, 47} <= located and any(t < 32 for t in located) and any(32 <= t < 47 for t in located)


def test_byte_kernel_bases_off_by_one_byte(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    n = k + m
    cells, _ = corrupt(codec, k, m, cell, seed=3)
    want_res, want_units, want_cells = R.correct_batch(codec, k, m, cells)
    flat = torch.full((cells.size + 64,), GUARD, dtype=torch.uint8, device=dev)
    flat[33:33 + cells.size] = torch.from_numpy(cells.reshape(-1)).to(dev)
    base = flat.data_ptr() + 33
    assert base % 16 == 1
    ptrs, strides = [base + i * cell for i in range(n)], [n * cell] * n
    res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
    units = torch.full((S,), FILL, dtype=torch.int32, device=dev)
    cod = coder(k, m)
    cod.scrub_device(ptrs, strides, cell, S, res.data_ptr(), stream())
    cod.scrub_correct_device(ptrs, strides, cell, S, res.data_ptr(), units.data_ptr(), stream())
    torch.cuda.synchronize()
    want_flat = np.full(cells.size + 64, GUARD, dtype=np.uint8)
    want_flat[33:33 + cells.size] = want_cells.reshape(-1)
    assert np.array_equal(as_u64(res), want_res)
    assert np.array_equal(units.cpu().numpy(), want_units)
    assert np.array_equal(flat.cpu().numpy(), want_flat)


def test_separate_allocations_and_strides(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    n = k + m
    cells, _ = corrupt(codec, k, m, cell, seed=5)
    want_res, want_units, want_cells = R.correct_batch(codec, k, m, cells)
    bufs = []
    for i in range(n):  # unit i in its own allocation, stride cell + 16 * i, 0xEE between the cells
        b = torch.full((S, cell + 16 * i), 0xEE, dtype=torch.uint8, device=dev)
        b[:, :cell] = torch.from_numpy(np.ascontiguousarray(cells[:, i])).to(dev)
        bufs.append(b)
    ptrs, strides = [b.data_ptr() for b in bufs], [cell + 16 * i for i in range(n)]
    res = torch.full((S, 2), -1, dtype=torch.int64, device=dev)
    units = torch.full((S,), FILL, dtype=torch.int32, device=dev)
    cod = coder(k, m)
    cod.scrub_device(ptrs, strides, cell, S, res.data_ptr(), stream())
    cod.scrub_correct_device(ptrs, strides, cell, S, res.data_ptr(), units.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(units.cpu().numpy(), want_units)
    for i, b in enumerate(bufs):
        got = b.cpu().numpy()
        assert np.array_equal(got[:, :cell], want_cells[:, i]), i
        assert (got[:, cell:] == 0xEE).all(), i


# ---- one dirty stripe is spread over the whole grid -----------------------------------

@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (10, 4)], ids=["rs-3-2", "rs-6-3", "rs-10-4"])
def test_one_dirty_stripe_spread_over_the_grid(dev, k, m):
    """Two stripes, one of them with a wholly random unit, and a cell of
    2 * waves wave-tiles + 16 bytes with the waves counted from the device (one
    block per CU): every wave of the grid takes at least two tiles of that
    stripe.  The truth is made on the device by encode_batch."""
    n = k + m
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    waves = cus * (8 if k > 6 else 4)
    cell = 2 * waves * TILE[k] + 16
    cod = coder(k, m)
    buf = torch.full((4, n, cell), GUARD, dtype=torch.uint8, device=dev)
    view = buf[1:3]
    view[:, :k] = torch.randint(0, 256, (2, k, cell), dtype=torch.uint8, device=dev)
    ptrs, strides = H.stripe_layout_ptrs(view, n)
    cod.encode_device(ptrs[:k], strides[:k], ptrs[k:], strides[k:], cell, 2, stream())
    want = buf.clone()
    for rnd, (st, t) in enumerate(((1, 1), (0, n - 1))):  # a data unit, then a parity unit
        view[st, t] ^= torch.randint(1, 256, (cell,), dtype=torch.uint8, device=dev)
        units = torch.full((2,), FILL, dtype=torch.int32, device=dev)
        res = H.scrub_batch(cod, view)
        H.scrub_correct_batch(cod, view, res, units)
        again = H.scrub_batch(cod, view)
        torch.cuda.synchronize()
        got = as_u64(res)
        assert int(got[st, 1]) == cell and not got[1 - st].any(), rnd
        assert H.scrub_verdict(int(got[st, 0]), cell, n) == (H.HEC_SCRUB_LOCATED, t), rnd
        assert units.cpu().tolist() == ([R.CLEAN, t] if st else [t, R.CLEAN]), rnd
        assert torch.equal(buf, want), rnd
        assert not as_u64(again).any(), rnd


# ---- stripe * stride past 4 GiB ----------------------------------------------------------

def test_stripe_stride_past_4gib(dev):
    """17 stripes 2^28 bytes apart: stripe 16 begins 2^32 bytes after stripe 0.
    Once with 16-byte aligned bases (the register kernel), once with every
    base one byte on (the byte kernel)."""
    codec, k, m, cell = "rs", 6, 3, 4112
    n, stripes, stride = k + m, 17, 1 << 28
    cells = truth(codec, k, m, stripes, cell).copy()
    cells[0, 2, 5] ^= 0x01
    cells[15, 7, cell - 1] ^= 0x40
    cells[16, 0, 0] ^= 0x80
    cells[16, 0, 4100] ^= 0x03
    want_res, want_units, want_cells = R.correct_batch(codec, k, m, cells)
    assert want_units.tolist() == [2] + [R.CLEAN] * 14 + [7, 0]
    assert np.array_equal(want_cells, truth(codec, k, m, stripes, cell))
    big = torch.empty(16 * stride + n * cell + 32, dtype=torch.uint8, device=dev)  # only the cells are written
    image = torch.from_numpy(cells).to(dev)
    cod = coder(k, m)
    for off in (0, 1):
        base = big.data_ptr() + off
        assert base % 16 == off and 16 * stride >= 1 << 32
        for st in range(stripes):
            big[st * stride + off:st * stride + off + n * cell].copy_(image[st].reshape(-1))
        ptrs, strides = [base + i * cell for i in range(n)], [stride] * n
        res = torch.full((stripes, 2), -1, dtype=torch.int64, device=dev)
        units = torch.full((stripes,), FILL, dtype=torch.int32, device=dev)
        cod.scrub_device(ptrs, strides, cell, stripes, res.data_ptr(), stream())
        cod.scrub_correct_device(ptrs, strides, cell, stripes, res.data_ptr(), units.data_ptr(), stream())
        torch.cuda.synchronize()
        assert np.array_equal(as_u64(res), want_res), off
        assert units.cpu().tolist() == want_units.tolist(), off
        for st in range(stripes):
            got = big[st * stride + off:st * stride + off + n * cell].cpu().numpy()
            assert np.array_equal(got, want_cells[st].reshape(-1)), (off, st)
    del big


# ---- scrub, correct, scrub on one stream ----------------------------------------------------

@pytest.mark.parametrize("k,m,cell", [(6, 3, 4096 + 512), (6, 3, 4112), (10, 4, 2048 + 512)],
                         ids=["rs-6-3-4608", "rs-6-3-4112", "rs-10-4-2560"])
def test_scrub_correct_scrub_on_one_stream(dev, k, m, cell):
    """scrub_crc_batch, scrub_correct_batch, scrub_crc_batch on a non-default
    stream with no host synchronisation between them; one read-back at the
    end.  The sums are the truth's: a corrected unit verifies again."""
    codec, n = "rs", k + m
    cod = coder(k, m)
    cells, _ = corrupt(codec, k, m, cell, seed=7)
    want_res, want_units, want_cells = R.correct_batch(codec, k, m, cells)
    clean = torch.from_numpy(truth(codec, k, m, S, cell).copy()).to(dev)
    sums = H.checksum_batch(cod, clean)
    buf, view = guarded(cells, dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        units = torch.full((S,), FILL, dtype=torch.int32, device=dev)
        first, bad1 = H.scrub_crc_batch(cod, view, sums, stream=st)
        H.scrub_correct_batch(cod, view, first, units, stream=st)
        second, bad2 = H.scrub_crc_batch(cod, view, sums, stream=st)
    st.synchronize()
    got_units = units.cpu().numpy()
    assert np.array_equal(got_units, want_units)
    assert np.array_equal(as_u64(first), want_res)
    after, flags, got = as_u64(second), bad2.cpu().numpy(), buf.cpu().numpy()
    assert np.array_equal(got, with_guards(want_cells))
    assert (got_units >= 0).sum() >= n and (got_units == R.UNLOCATED).any()
    for s in range(S):
        if got_units[s] >= 0:
            assert tuple(after[s]) == (0, 0) and not flags[s].any(), s
        elif got_units[s] == R.UNLOCATED:
            assert np.array_equal(got[1 + s], cells[s]), s  # bit-identical to its corrupted state
            assert tuple(after[s]) == tuple(want_res[s]) and flags[s].any(), s
        else:
            assert tuple(after[s]) == (0, 0) and not flags[s].any() and not bad1.cpu().numpy()[s].any(), s


# ---- stream capture -----------------------------------------------------------------------------

def test_graph_capture_replay(dev):
    """torch.cuda.graph around scrub, correct, scrub for (6,3) and (10,4),
    replayed twice with the cells corrupted differently before each replay."""
    shapes = [(6, 3), (10, 4)]
    cods = [coder(k, m) for k, m in shapes]
    cell = [TILE[k] + 16 for k, _ in shapes]
    static = [torch.full((S + 2, k + m, c), GUARD, dtype=torch.uint8, device=dev) for (k, m), c in zip(shapes, cell)]
    first = [torch.full((S, 2), -1, dtype=torch.int64, device=dev) for _ in shapes]
    second = [torch.full((S, 2), -1, dtype=torch.int64, device=dev) for _ in shapes]
    units = [torch.full((S,), FILL, dtype=torch.int32, device=dev) for _ in shapes]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for cod, (k, m), c, buf, r1, r2, u in zip(cods, shapes, cell, static, first, second, units):
            ptrs, strides = H.stripe_layout_ptrs(buf[1:-1], k + m)
            cod.scrub_device(ptrs, strides, c, S, r1.data_ptr(), stream())
            cod.scrub_correct_device(ptrs, strides, c, S, r1.data_ptr(), u.data_ptr(), stream())
            cod.scrub_device(ptrs, strides, c, S, r2.data_ptr(), stream())
    for rep in range(2):
        want = []
        for (k, m), c, buf, r1, r2, u in zip(shapes, cell, static, first, second, units):
            cells, _ = corrupt("rs", k, m, c, seed=11 + rep)
            want.append((cells,) + R.correct_batch("rs", k, m, cells))
            buf[1:-1] = torch.from_numpy(cells).to(dev)
            r1.fill_(-1)
            r2.fill_(-1)
            u.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for (k, m), c, buf, r1, r2, u, (cells, want_res, want_units, want_cells) in zip(shapes, cell, static, first,
                                                                                        second, units, want):
            assert np.array_equal(as_u64(r1), want_res), (rep, k)
            assert np.array_equal(u.cpu().numpy(), want_units), (rep, k)
            assert np.array_equal(buf.cpu().numpy(), with_guards(want_cells)), (rep, k)
            assert np.array_equal(as_u64(r2), R.correct_batch("rs", k, m, want_cells)[0]), (rep, k)
            assert not as_u64(r2)[want_units >= 0].any(), (rep, k)
    assert not np.array_equal(want[0][2], R.correct_batch("rs", 6, 3, corrupt("rs", 6, 3, cell[0], seed=11)[0])[1])
    del g


# ---- status codes ----------------------------------------------------------------------------------

def test_zero_stripes_and_errors_queue_nothing(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    n = k + m
    cells = truth(codec, k, m, S, cell).copy()
    cells[3, 2, 9] ^= 1
    buf, view = guarded(cells, dev)
    cod = coder(k, m)
    res = H.scrub_batch(cod, view)
    ptrs, strides = H.stripe_layout_ptrs(view, n)
    units = torch.full((S + 1,), FILL, dtype=torch.int32, device=dev)
    lib = cod._lib

    def call(h, p, cell_len, results, d_units, stripes=S, strides_=strides):
        return lib.hec_scrub_correct_device(h, H._pp(p) if p is not None else None,
                                            H._sp(strides_) if strides_ is not None else None, cell_len, stripes,
                                            ctypes.c_void_p(results), ctypes.c_void_p(d_units),
                                            ctypes.c_void_p(stream()))

    assert call(cod.handle, ptrs, cell, res.data_ptr(), units.data_ptr(), stripes=0) == H.HEC_OK
    for t in (0, k, n - 1):
        assert call(cod.handle, [0 if i == t else p for i, p in enumerate(ptrs)], cell, res.data_ptr(),
                    units.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(None, ptrs, cell, res.data_ptr(), units.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, None, cell, res.data_ptr(), units.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, res.data_ptr(), units.data_ptr(), strides_=None) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, 0, res.data_ptr(), units.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, 0, units.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, res.data_ptr(), 0) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, res.data_ptr() + 4, units.data_ptr()) == H.HEC_ERR_INVALID_ARG  # 8-byte alignment
    assert call(cod.handle, ptrs, cell, res.data_ptr(), units.data_ptr() + 2) == H.HEC_ERR_INVALID_ARG  # 4-byte alignment
    host = H.Coder(k, m, H.HEC_DEVICE_HOST)
    assert call(host.handle, ptrs, cell, res.data_ptr(), units.data_ptr()) == H.HEC_ERR_DEVICE
    with pytest.raises(H.DeviceError):
        host.scrub_correct_device(ptrs, strides, cell, S, res.data_ptr(), units.data_ptr(), stream())
    host.close()
    torch.cuda.synchronize()
    assert (units == FILL).all()  # the pre-fill is untouched: nothing was queued
    assert np.array_equal(buf.cpu().numpy(), with_guards(cells))
    # 4-byte aligned is enough for d_units; the entry past the batch stays
    assert call(cod.handle, ptrs, cell, res.data_ptr(), units.data_ptr() + 4) == H.HEC_OK
    torch.cuda.synchronize()
    assert units.cpu().tolist() == [FILL] + [R.CLEAN] * 3 + [2] + [R.CLEAN] * (S - 4)
    assert np.array_equal(buf.cpu().numpy(), with_guards(truth(codec, k, m, S, cell)))
