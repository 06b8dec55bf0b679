"""Stripe scrub on the GPU (hec_scrub_device: the gf_scrub register kernel and
the byte-granular gf_scrub_bytes).  Expected results come from _ref_batch
below, a numpy restatement of the definition over the oracle's matrix and
product table (syndromes s_j = sum_i P[j][i] u_i ^ u_{k+j}; ruled_out bit t
when some position's syndrome vector has a non-zero 2x2 minor against column t
of H = [P | I]); the WHOLE result array is compared, exactly, so a count that
lands on the wrong stripe or a lane past the cell that is counted shows as
well as a wrong mask.  Every result buffer is handed in filled with 0xFF: the
call zeroes it itself.

Which kernel each group of tests reaches (ScrubFn in csrc/ec_scrub.hip
builds gf_scrub<K, M, U, BS, WQ> for K in {2, 3, 6, 10} x M in {1, 2, 3, 4},
each with the work queue, WQ > 0, and in the fixed tile order, WQ == 0; a
kernel added there gets its row here):

  group (test)                                  kernels
  --------------------------------------------  ---------------------------------
  REGISTER (test_clean_batch_writes_zeros,      gf_scrub<K, M, .., WQ > 0>, all 16
    test_corruptions_equal_reference)             (K, M) with rs; M == 1 again with
                                                  xor at K = 2, 3, 6, 10; rs-legacy
                                                  at (3,2), (6,3), (10,4); cells
                                                  around the wave-tile for (6,3)
                                                  and (10,4)
  BYTE (the same two tests, test_generic_*)     gf_scrub_bytes: k outside the fast
                                                  set ((5,3), xor (5,1)), an odd
                                                  cell length, bases off by a byte
  test_gpu_scrub_variants.py:
    test_byte_kernel_shapes                     gf_scrub_bytes at (4,8), (32,16),
                                                  (6,5) (there because of m alone),
                                                  (1,2), xor (5,1)
    test_more_tiles_than_waves                  gf_scrub<3,2 / 6,3 / 10,4, WQ > 0>,
                                                  every wave through the tile loop
                                                  at least twice
    test_stripe_stride_past_4gib                gf_scrub<6,3, WQ > 0> and
                                                  gf_scrub_bytes, stripe offsets
                                                  of 2^32 and more
    test_three_streams_at_once                  gf_scrub<6,3, WQ > 0>, the stream
                                                  counter sets of three streams
    test_graph_capture_replay                   gf_scrub<6,3> and <10,4>, WQ > 0 on
                                                  graph counter sets
    test_fixed_tile_order_in_child_process      gf_scrub<K, M, WQ == 0>, all 16
      (scrub_fixed_order_child.py)                (K, M), and the fixed-order
                                                  gf_matmul kernels behind encode,
                                                  decode and reconstruct, once the
                                                  graph pool is used up
"""
import ctypes

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S = 37  # leaves a remainder stripe after the 4-stripe tile groups
TILE = {2: 4096, 3: 4096, 6: 4096, 10: 2048}  # bytes of a wave-tile of the register kernel, by k
# (codec, k, m, cell_len, wave-tile bytes).  The register kernel: cells around
# the wave-tiles of (6,3) and (10,4), then one wave-tile + 16 bytes at all 16
# (k, m) it is built for, the M == 1 kernels again with xor, and rs-legacy
REGISTER = [("rs", 6, 3, 16, 4096), ("rs", 6, 3, 4096, 4096), ("rs", 6, 3, 12336, 4096),
            ("rs", 10, 4, 16, 2048), ("rs", 10, 4, 2048, 2048), ("rs", 10, 4, 6160, 2048)]
REGISTER += [("rs", k, m, TILE[k] + 16, TILE[k]) for k in (2, 3, 6, 10) for m in (1, 2, 3, 4)]
REGISTER += [("xor", k, 1, TILE[k] + 16, TILE[k]) for k in (2, 3, 6, 10)]
REGISTER += [("rs-legacy", k, m, TILE[k] + 16, TILE[k]) for k, m in ((3, 2), (6, 3), (10, 4))]
# The byte kernel: k = 5 is not a shape of the register kernel, so this case
# has always run gf_scrub_bytes (the other byte-kernel cases are the
# test_generic_* below and test_gpu_scrub_variants.py)
BYTE = [("xor", 5, 1, 4112, 4096)]
FAST = REGISTER + BYTE
IDS = [f"{c}-{k}-{m}-{cell}" for c, k, m, cell, _ in FAST]
assert len(set(IDS)) == len(IDS) == 6 + 16 + 4 + 3 + 1


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


def consistent_stripes(codec, k, m, stripes, cell):
    """A fresh, writable [stripes, k+m, cell]: random data and the oracle's
    parity rows applied to it (the same bytes for the same arguments)."""
    rng = np.random.default_rng(104729 * k + 31 * m + stripes + cell + len(codec))
    t = np.empty((stripes, k + m, cell), dtype=np.uint8)
    t[:, :k] = rng.integers(0, 256, size=(stripes, k, cell), dtype=np.uint8)
    flat = [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)]
    par = O.matmul_shards(O.codec_matrix(codec, k, m)[k:], flat)
    for j in range(m):
        t[:, k + j] = par[j].reshape(stripes, cell)
    return t


def truth(codec, k, m, stripes, cell):
    """Consistent stripes [stripes, k+m, cell], computed once per shape,
    shared, read-only."""
    key = (codec, k, m, stripes, cell)
    if key not in _truth:
        t = consistent_stripes(codec, k, m, stripes, cell)
        t.setflags(write=False)
        _truth[key] = t
    return _truth[key]


def _ref_batch(codec, k, m, cells):
    """uint64 [stripes, 2] of (ruled_out, bad_bytes) by the definition."""
    C = O.codec_matrix(codec, k, m)
    P = np.array(C[k:], dtype=np.uint8)
    Hm = np.concatenate([P, np.eye(m, dtype=np.uint8)], axis=1)
    s = np.ascontiguousarray(cells[:, k:].transpose(1, 0, 2)).copy()  # [m, stripes, cell]
    for j in range(m):
        for i in range(k):
            s[j] ^= O.MUL_TABLE[P[j, i]][cells[:, i]]
    out = np.zeros((cells.shape[0], 2), dtype=np.uint64)
    for st in np.nonzero(s.any(axis=(0, 2)))[0]:
        bad = np.nonzero(s[:, st].any(axis=0))[0]
        sb = s[:, st][:, bad]
        ruled = 0
        for t in range(k + m):
            for i in range(m):
                for j in range(i + 1, m):
                    if (O.MUL_TABLE[Hm[j, t]][sb[i]] ^ O.MUL_TABLE[Hm[i, t]][sb[j]]).any():
                        ruled |= 1 << t
        out[st] = (ruled, len(bad))
    return out


def stream():
    return torch.cuda.current_stream().cuda_stream


def prefilled(stripes, dev):
    return torch.full((max(stripes, 1), 2), -1, dtype=torch.int64, device=dev)  # 0xFF in every byte


def as_u64(res, stripes):
    return res.cpu().numpy().view(np.uint64)[:stripes]


def scrub(cod, cells, dev):
    """One hec_scrub_device call over a numpy [stripes, k+m, cell] image in the
    packed layout, into a 0xFF-filled buffer."""
    buf = torch.from_numpy(np.array(cells)).to(dev)  # a writable copy: the shared originals are read-only
    stripes, n, cell = cells.shape
    res = prefilled(stripes, dev)
    ptrs, strides = H.stripe_layout_ptrs(buf, n)
    cod.scrub_device(ptrs, strides, cell, stripes, res.data_ptr(), stream())
    torch.cuda.synchronize()
    return as_u64(res, stripes)


def single_byte_corruptions(cells, k, m, tile):
    """One corrupt byte in each of a dozen stripes (in place): the offsets 0,
    15, 16, tile-1, tile, cell-16, cell-1 (those inside the cell), the first
    and last data and parity units."""
    cell = cells.shape[2]
    offsets = sorted({o for o in (0, 15, 16, tile - 1, tile, cell - 16, cell - 1) if 0 <= o < cell})
    units = [0, k - 1, k, k + m - 1]
    stripes = [0, 1, 2, 3, 5, 8, 13, 21, 33, 34, 35, 36]
    for x, st in enumerate(stripes):
        cells[st, units[(x + x // 4) % 4], offsets[x % len(offsets)]] ^= 1 + x
    return stripes


def assorted_corruptions(codec, k, m, cell, tile):
    """The test image of one shape: a dozen single-byte stripes, one stripe
    with 200 corrupt positions of one unit spread over all tiles (cells of 200
    bytes and more), one with a wholly random unit, two units at two positions,
    two units at one position.  Returns (cells, notes)."""
    cells = truth(codec, k, m, S, cell).copy()
    rng = np.random.default_rng(cell + k)
    notes = {"single": single_byte_corruptions(cells, k, m, tile)}
    if cell >= 200:
        spread = np.unique(np.linspace(0, cell - 1, 50).astype(np.int64))  # every tile, first and last byte
        rest = rng.permutation(np.setdiff1d(np.arange(cell), spread))[:200 - len(spread)]
        pos = np.concatenate([spread, rest])
        assert len(np.unique(pos)) == 200 and len(np.unique(pos // tile)) == (cell + tile - 1) // tile
        cells[4, k - 2, pos] ^= rng.integers(1, 256, size=200, dtype=np.uint8)
        notes["many"] = (4, k - 2)
    cells[6, k] = rng.integers(0, 256, size=cell, dtype=np.uint8)
    notes["random"] = (6, k)
    cells[7, 1, 0] ^= 0x21
    cells[7, k + m - 1, cell - 1] ^= 0x80
    notes["two_positions"] = 7
    cells[9, 0, cell // 2] ^= 0x35
    cells[9, k - 1, cell // 2] ^= 0xC1
    notes["one_position"] = 9
    return cells, notes


@pytest.mark.parametrize("codec,k,m,cell,tile", FAST, ids=IDS)
def test_clean_batch_writes_zeros(dev, codec, k, m, cell, tile):
    got = scrub(coder(k, m, codec), truth(codec, k, m, S, cell), dev)
    assert not got.any()


@pytest.mark.parametrize("codec,k,m,cell,tile", FAST, ids=IDS)
def test_corruptions_equal_reference(dev, codec, k, m, cell, tile):
    cells, notes = assorted_corruptions(codec, k, m, cell, tile)
    want = _ref_batch(codec, k, m, cells)
    got = scrub(coder(k, m, codec), cells, dev)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    n = k + m
    full = (1 << n) - 1
    # the closed forms the definition gives, checked on the reference itself
    for st in notes["single"]:
        assert want[st, 1] == 1 and (m == 1 or bin(int(want[st, 0]) ^ full).count("1") == 1)
    if "many" in notes:
        st, unit = notes["many"]
        assert int(got[st, 1]) == 200
        assert H.scrub_verdict(int(got[st, 0]), 200, n) == ((H.HEC_SCRUB_LOCATED, unit) if m > 1 else
                                                            (H.HEC_SCRUB_AMBIGUOUS, None))
    st, unit = notes["random"]
    if m > 1:
        assert H.scrub_verdict(int(got[st, 0]), int(got[st, 1]), n) == (H.HEC_SCRUB_LOCATED, unit)
    assert tuple(got[notes["two_positions"]]) == (full if m > 1 else 0, 2)
    if m >= 3:
        assert tuple(got[notes["one_position"]]) == (full, 1)
    if m == 1:
        assert not got[:, 0].any()  # one parity cannot locate


def test_separate_allocations_and_strides(dev):
    codec, k, m, cell, tile = "rs", 6, 3, 4112, 4096
    cells, _ = assorted_corruptions(codec, k, m, cell, tile)
    want = _ref_batch(codec, k, m, cells)
    bufs = []
    for i in range(k + m):  # unit i in its own allocation, stride cell + 16 * i
        b = torch.full((S, cell + 16 * i), 0xEE, dtype=torch.uint8, device=dev)
        b[:, :cell] = torch.from_numpy(np.ascontiguousarray(cells[:, i])).to(dev)
        bufs.append(b)
    res = prefilled(S, dev)
    coder(k, m).scrub_device([b.data_ptr() for b in bufs], [cell + 16 * i for i in range(k + m)], cell, S,
                             res.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(res, S), want)


def test_zero_and_one_stripe(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    cells = truth(codec, k, m, 1, cell).copy()
    cells[0, 7, 4100] ^= 4
    buf = torch.from_numpy(cells).to(dev)
    ptrs, strides = H.stripe_layout_ptrs(buf, k + m)
    res = prefilled(1, dev)
    coder(k, m).scrub_device(ptrs, strides, cell, 0, res.data_ptr(), stream())
    torch.cuda.synchronize()
    assert (res == -1).all()  # nothing queued
    coder(k, m).scrub_device(ptrs, strides, cell, 1, res.data_ptr(), stream())
    torch.cuda.synchronize()
    assert as_u64(res, 1).tolist() == [[0x1FF & ~(1 << 7), 1]]
    assert np.array_equal(as_u64(res, 1), _ref_batch(codec, k, m, cells))


def test_scrub_batch_wrapper(dev):
    codec, k, m, cell, tile = "rs", 10, 4, 2064, 2048
    cells, _ = assorted_corruptions(codec, k, m, cell, tile)
    out = H.scrub_batch(coder(k, m), torch.from_numpy(cells).to(dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.int64 and tuple(out.shape) == (S, 2)
    assert np.array_equal(as_u64(out, S), _ref_batch(codec, k, m, cells))


# ---- the byte-granular kernel --------------------------------------------------

def test_generic_other_k(dev):
    codec, k, m, cell = "rs", 5, 3, 4112
    cells, _ = assorted_corruptions(codec, k, m, cell, 4096)
    assert np.array_equal(scrub(coder(k, m), cells, dev), _ref_batch(codec, k, m, cells))
    assert not scrub(coder(k, m), truth(codec, k, m, S, cell), dev).any()


def test_generic_odd_cell_len(dev):
    codec, k, m, cell = "rs", 6, 3, 4099
    cells, _ = assorted_corruptions(codec, k, m, cell, 4096)
    assert np.array_equal(scrub(coder(k, m), cells, dev), _ref_batch(codec, k, m, cells))
    assert not scrub(coder(k, m), truth(codec, k, m, S, cell), dev).any()


def test_generic_bases_offset_by_one_byte(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    cells, _ = assorted_corruptions(codec, k, m, cell, 4096)
    flat = torch.full((S * (k + m) * cell + 16,), 0xEE, dtype=torch.uint8, device=dev)
    flat[1:1 + cells.size] = torch.from_numpy(cells.reshape(-1)).to(dev)
    base = flat.data_ptr() + 1
    res = prefilled(S, dev)
    coder(k, m).scrub_device([base + i * cell for i in range(k + m)], [(k + m) * cell] * (k + m), cell, S,
                             res.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(res, S), _ref_batch(codec, k, m, cells))


# ---- the stream's counter sets, the repair loop, errors --------------------------

def test_back_to_back_calls_on_one_stream(dev):
    # consecutive launches on a stream alternate between its two counter sets
    codec, k, m, cell, tile = "rs", 6, 3, 12336, 4096
    cells, _ = assorted_corruptions(codec, k, m, cell, tile)
    want = _ref_batch(codec, k, m, cells)
    dirty = torch.from_numpy(cells).to(dev)
    clean = torch.from_numpy(truth(codec, k, m, S, cell).copy()).to(dev)
    res = [prefilled(S, dev) for _ in range(3)]
    for r, buf in zip(res, (dirty, clean, dirty)):
        ptrs, strides = H.stripe_layout_ptrs(buf, k + m)
        coder(k, m).scrub_device(ptrs, strides, cell, S, r.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(res[0], S), want)
    assert not as_u64(res[1], S).any()
    assert np.array_equal(as_u64(res[2], S), want)


def test_scrub_reconstruct_scrub(dev):
    """The repair loop: every unit index corrupt in one stripe, located by the
    scrub, rebuilt in place by the mixed reconstruction, confirmed by a
    second scrub."""
    codec, k, m, cell = "rs", 6, 3, 4112
    n = k + m
    full = (1 << n) - 1
    orig = truth(codec, k, m, S, cell)
    cells = orig.copy()
    rng = np.random.default_rng(63)
    hit = {4 * u + 1: u for u in range(n)}  # stripe -> its corrupt unit (stripes 1, 5, ..., 33)
    for st, u in hit.items():
        if u % 2:
            cells[st, u] = rng.integers(0, 256, size=cell, dtype=np.uint8)
        else:
            cells[st, u, rng.choice(cell, size=5, replace=False)] ^= 0x5A
    buf = torch.from_numpy(cells).to(dev)
    cod = coder(k, m)
    first = H.scrub_batch(cod, buf)
    torch.cuda.synchronize()
    masks = []
    for st, (ruled, bad) in enumerate(as_u64(first, S).tolist()):
        verdict, unit = H.scrub_verdict(ruled, bad, n)
        if st in hit:
            assert (verdict, unit) == (H.HEC_SCRUB_LOCATED, hit[st]), st
            masks.append(full & ~(1 << unit))
        else:
            assert verdict == H.HEC_SCRUB_CLEAN, st
            masks.append(full)
    H.reconstruct_batch_mixed(cod, buf, masks)
    second = H.scrub_batch(cod, buf)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), torch.from_numpy(orig.copy()))
    assert not as_u64(second, S).any()


def test_errors_queue_nothing(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    buf = torch.from_numpy(truth(codec, k, m, S, cell).copy()).to(dev)
    buf[3, 2, 9] ^= 1
    ptrs, strides = H.stripe_layout_ptrs(buf, k + m)
    res = prefilled(S, dev)
    cod = coder(k, m)
    lib = cod._lib

    def call(h, p, cell_len, results):
        return lib.hec_scrub_device(h, H._pp(p), H._sp(strides), cell_len, S, ctypes.c_void_p(results),
                                    ctypes.c_void_p(stream()))

    for t in (0, k, k + m - 1):
        assert call(cod.handle, [0 if i == t else p for i, p in enumerate(ptrs)], cell,
                    res.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, 0, res.data_ptr()) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, 0) == H.HEC_ERR_INVALID_ARG
    assert call(cod.handle, ptrs, cell, res.data_ptr() + 4) == H.HEC_ERR_INVALID_ARG  # 8-byte alignment
    host = H.Coder(k, m, H.HEC_DEVICE_HOST)
    assert call(host.handle, ptrs, cell, res.data_ptr()) == H.HEC_ERR_DEVICE
    with pytest.raises(H.DeviceError):
        host.scrub_device(ptrs, strides, cell, S, res.data_ptr(), stream())
    host.close()
    torch.cuda.synchronize()
    assert (res == -1).all()  # the pre-fill is untouched: nothing was queued
