"""Stripe scrub on the GPU, the parts of csrc/ec_scrub.hip that the shapes of
test_gpu_scrub.py leave out (its module docstring has the table of which
kernel each group reaches): the byte kernel with more than 4 parity units and
units numbered 32 and up, batches with more wave-tiles than the device has
waves, stripe offsets past 4 GiB, three streams at once, stream capture and
replay, and (in a child process, since it uses up the device's graph counter
sets for good) the fixed tile order every launcher falls back to.

The method is that of test_gpu_scrub.py: expected values from its _ref_batch,
result buffers handed in filled with 0xFF, the whole [S, 2] array compared
exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hdfs_native_ec as H
from test_gpu_scrub import (S, TILE, _ref_batch, as_u64, assorted_corruptions, coder, consistent_stripes, dev,  # noqa: F401
                            prefilled, scrub, stream, truth)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))


def launch(cod, buf, res, stripes=None, st=None):
    """hec_scrub_device over a device tensor [stripes, k+m, cell] into res, on
    the stream st (default: the current one); asynchronous."""
    n, cell = buf.shape[1], buf.shape[2]
    ptrs, strides = H.stripe_layout_ptrs(buf, n)
    cod.scrub_device(ptrs, strides, cell, buf.shape[0] if stripes is None else stripes, res.data_ptr(),
                     stream() if st is None else st.cuda_stream)


def loop_waves(k):
    """Waves the work-queue launch of gf_scrub keeps resident: one block per
    CU, of 4 waves up to k = 6 and of 8 waves for k = 10."""
    return torch.cuda.get_device_properties(0).multi_processor_count * (8 if k == 10 else 4)


def loop_shape(k):
    """(stripes, cell) with 4 wave-tiles per stripe and more than twice as many
    tiles as resident waves: every wave takes the tile loop at least twice."""
    return -(-2 * loop_waves(k) // 4) + 1, 3 * TILE[k] + 16


def spread_corruptions(cells, k, m, seed):
    """About two dozen corrupt stripes spread over a batch of any size (in
    place): single bytes in the first and the last stripe, either side of
    multiples of 4 (the tile-order group) and at random stripes, in every tile
    of a stripe; one wholly random unit; one stripe hit in two units at
    positions in different tiles.  Returns notes as assorted_corruptions."""
    stripes, n, cell = cells.shape
    tile = TILE.get(k, 4096)
    rng = np.random.default_rng(seed)
    mid, late = stripes // 2 // 4 * 4, 3 * stripes // 4 // 4 * 4
    fixed = [0, 3, 4, 5, mid - 1, mid, mid + 1, late - 1, late, late + 1, stripes - 2, stripes - 1]
    fixed = sorted({s for s in fixed if 0 <= s < stripes})
    rest = np.setdiff1d(np.arange(stripes), fixed)
    extra = sorted(int(s) for s in rng.choice(rest, size=min(12, len(rest) - 2), replace=False))
    offsets = sorted({o for o in (0, 15, 16, tile - 1, tile, 2 * tile + 5, 3 * tile - 16, cell - 16, cell - 1)
                      if 0 <= o < cell})
    single = fixed + extra[:-2]
    for x, st in enumerate(single):
        cells[st, int(rng.integers(0, n)), offsets[x % len(offsets)]] ^= 1 + x % 255
    notes = {"single": single, "random": (extra[-2], int(rng.integers(0, n))), "two_units": extra[-1]}
    st, unit = notes["random"]
    cells[st, unit] ^= rng.integers(1, 256, size=cell, dtype=np.uint8)  # every byte of the unit differs
    cells[extra[-1], 0, 7] ^= 0x21
    cells[extra[-1], n - 1, cell - 3] ^= 0x80
    return notes


def check_notes(got, want, notes, k, m, cell):
    """The closed forms of the definition at the stripes spread_corruptions
    hit, on the reference itself; then the device's words against it."""
    n, full = k + m, (1 << (k + m)) - 1
    hit = set(notes["single"]) | {notes["random"][0], notes["two_units"]}
    assert sorted(np.nonzero(want[:, 1])[0].tolist()) == sorted(hit)
    for st in notes["single"]:
        assert want[st, 1] == 1 and (m == 1 or bin(int(want[st, 0]) ^ full).count("1") == 1)
    st, unit = notes["random"]
    assert want[st, 1] == cell
    if m > 1:
        assert H.scrub_verdict(int(want[st, 0]), cell, n) == (H.HEC_SCRUB_LOCATED, unit)
        assert tuple(want[notes["two_units"]]) == (full, 2)  # two units, two positions: every unit ruled out
    assert np.array_equal(got, want), (np.nonzero((got != want).any(axis=1))[0].tolist(),
                                       got[(got != want).any(axis=1)].tolist())


# ---- more tiles than waves: the second pass of the tile loop -------------------

@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (10, 4)], ids=["rs-3-2", "rs-6-3", "rs-10-4"])
def test_more_tiles_than_waves(dev, k, m):
    """4 wave-tiles per stripe and S = ceil(2 * waves / 4) + 1 stripes, with the
    waves counted from the device: every wave fetches from its counter again
    after its first tile, and the last fetches land past the end."""
    stripes, cell = loop_shape(k)
    assert 4 * stripes > 2 * loop_waves(k)
    cells = consistent_stripes("rs", k, m, stripes, cell)
    cod = coder(k, m)
    assert not scrub(cod, cells, dev).any()
    notes = spread_corruptions(cells, k, m, seed=7 * k + m)
    assert len(notes["single"]) + 2 >= min(20, stripes - 2)
    check_notes(scrub(cod, cells, dev), _ref_batch("rs", k, m, cells), notes, k, m, cell)


# ---- the byte kernel: wide m, units numbered 32 and up, dispatch by m ------------

# (codec, k, m, cell).  (6,5) at a 16-byte-aligned cell has a k of the register
# kernel and is here because of m alone; xor (5,1) because of k
BYTE_SHAPES = [("rs", 4, 8, 4099), ("rs", 32, 16, 4099), ("rs", 6, 5, 4112), ("rs", 1, 2, 4099), ("xor", 5, 1, 4112)]


@pytest.mark.parametrize("codec,k,m,cell", BYTE_SHAPES, ids=[f"{c}-{k}-{m}-{cell}" for c, k, m, cell in BYTE_SHAPES])
def test_byte_kernel_shapes(dev, codec, k, m, cell):
    n, full = k + m, (1 << (k + m)) - 1
    cells, _ = assorted_corruptions(codec, k, m, cell, 4096)
    # single bytes in the first and last data unit and the first, a middle
    # and the last parity unit, on stripes that hold nothing else
    alone = {10: 0, 11: k - 1, 12: k, 14: k + m // 2, 15: n - 1}
    for x, (st, unit) in enumerate(alone.items()):
        cells[st, unit, (0, 255, 256, 4095, cell - 1)[x]] ^= 0x10 << (x % 4)
    want = _ref_batch(codec, k, m, cells)
    cod = coder(k, m, codec)
    got = scrub(cod, cells, dev)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for st, unit in alone.items():
        assert tuple(want[st]) == (full & ~(1 << unit) if m > 1 else 0, 1)
    if (k, m) == (32, 16):
        # the high half of the 64-bit words: the reference has bits 32..47, and
        # the device's words locate units on both sides of bit 32
        assert int(np.bitwise_or.reduce(want[:, 0])) >> 32 == 0xFFFF
        for st, unit in alone.items():
            assert H.scrub_verdict(int(got[st, 0]), int(got[st, 1]), 48) == (H.HEC_SCRUB_LOCATED, unit)
        assert sorted(alone.values()) == [0, 31, 32, 40, 47]
    assert not scrub(cod, truth(codec, k, m, S, cell), dev).any()


# ---- stripe * stride past 4 GiB --------------------------------------------------

def test_stripe_stride_past_4gib(dev):
    """17 stripes 2^28 bytes apart: stripe 16 begins 2^32 bytes after stripe 0
    (a product kept in 32 bits would read stripe 0 again).  Once with 16-byte
    aligned bases (the register kernel), once with every base one byte on (the
    byte kernel)."""
    codec, k, m, cell = "rs", 6, 3, 4112
    n, stripes, stride = k + m, 17, 1 << 28
    cells = truth(codec, k, m, stripes, cell).copy()
    cells[0, 2, 5] ^= 0x01
    cells[15, 7, cell - 1] ^= 0x40
    cells[16, 0, 0] ^= 0x80
    cells[16, 0, 4100] ^= 0x03
    want = _ref_batch(codec, k, m, cells)
    assert want[:, 1].tolist() == [1] + [0] * 14 + [1, 2]
    assert H.scrub_verdict(int(want[16, 0]), 2, n) == (H.HEC_SCRUB_LOCATED, 0)
    big = torch.empty(16 * stride + n * cell + 32, dtype=torch.uint8, device=dev)  # only the cells are written
    image = torch.from_numpy(cells).to(dev)
    for off in (0, 1):
        base = big.data_ptr() + off
        assert base % 16 == off and 16 * stride >= 1 << 32
        for st in range(stripes):
            big[st * stride + off:st * stride + off + n * cell].copy_(image[st].reshape(-1))
        res = prefilled(stripes, dev)
        coder(k, m).scrub_device([base + i * cell for i in range(n)], [stride] * n, cell, stripes, res.data_ptr(),
                                 stream())
        torch.cuda.synchronize()
        got = as_u64(res, stripes)
        assert np.array_equal(got, want), (off, got.tolist(), want.tolist())
    del big


# ---- streams and stream capture ----------------------------------------------------

def test_three_streams_at_once(dev):
    """Three streams share one (6,3) coder and scrub an image each, all three
    launched before one synchronize, three rounds; every third launch of a
    stream (a different round for each) has a clean image.  The counter sets
    are per stream and the results are accumulated with atomics: every result
    equals its own reference."""
    codec, k, m = "rs", 6, 3
    stripes, cell = 149, 3 * TILE[k] + 16
    cod = coder(k, m)
    clean = consistent_stripes(codec, k, m, stripes, cell)
    d_clean = torch.from_numpy(clean).to(dev)
    dirty, want = [], []
    for i in range(3):
        cells = clean.copy()
        spread_corruptions(cells, k, m, seed=500 + i)
        want.append(_ref_batch(codec, k, m, cells))
        dirty.append(torch.from_numpy(cells).to(dev))
    assert not any(np.array_equal(want[i], want[j]) for i in range(3) for j in range(i))
    streams = [torch.cuda.Stream() for _ in range(3)]
    res = [prefilled(stripes, dev) for _ in range(3)]
    torch.cuda.synchronize()
    for rnd in range(3):
        for r in res:
            r.fill_(-1)
        torch.cuda.synchronize()
        for i, st in enumerate(streams):
            launch(cod, d_clean if (rnd + i) % 3 == 2 else dirty[i], res[i], st=st)
        torch.cuda.synchronize()
        for i in range(3):
            got = as_u64(res[i], stripes)
            if (rnd + i) % 3 == 2:
                assert not got.any(), (rnd, i)
            else:
                assert np.array_equal(got, want[i]), (rnd, i)


def test_graph_capture_replay(dev):
    """torch.cuda.graph around one scrub each of (6,3) and (10,4): the captured
    kernels count on graph counter sets, and those and the result words are
    zeroed by nodes of the graph at every replay (a missing one leaves 0xFF
    words on a clean replay; a captured hipMemsetAsync, which the library used
    before, left a 16-byte pattern of addresses in the words once other
    launches had gone by: the HIP runtime of the PyTorch ROCm 7.0 wheel
    replays it with a stale fill pattern).  Replays between direct scrubs on the same stream, and on
    a second stream while the first runs direct scrubs."""
    shapes = [(6, 3), (10, 4)]
    cods = [coder(k, m) for k, m in shapes]
    cell = [TILE[k] + 16 for k, _ in shapes]
    clean = [truth("rs", k, m, S, c).copy() for (k, m), c in zip(shapes, cell)]  # writable, for torch
    dirty, want = [], []
    for v in range(2):  # two dirty images per shape
        dirty.append([])
        want.append([])
        for (k, m), c, t in zip(shapes, cell, clean):
            cells = t.copy()
            spread_corruptions(cells, k, m, seed=900 + 10 * v + k)
            dirty[v].append(cells)
            want[v].append(_ref_batch("rs", k, m, cells))
    static = [torch.zeros(t.shape, dtype=torch.uint8, device=dev) for t in clean]
    res = [prefilled(S, dev) for _ in shapes]
    # the direct launches beside the replays: a larger (6,3) batch of its own
    d_stripes, d_cell = 149, 3 * TILE[6] + 16
    d_cells = consistent_stripes("rs", 6, 3, d_stripes, d_cell)
    spread_corruptions(d_cells, 6, 3, seed=77)
    d_want = _ref_batch("rs", 6, 3, d_cells)
    d_buf = torch.from_numpy(d_cells).to(dev)
    d_res = [prefilled(d_stripes, dev) for _ in range(2)]
    torch.cuda.synchronize()
    g0 = H.queue_stats(0)["graph_sets"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for cod, buf, r in zip(cods, static, res):
            launch(cod, buf, r)
    assert H.queue_stats(0)["graph_sets"] - g0 == 2  # both launches took the work queue
    other = torch.cuda.Stream()
    for rep in range(6):
        is_clean = rep % 2 == 1
        for i in range(2):
            static[i].copy_(torch.from_numpy(clean[i] if is_clean else dirty[rep // 2 % 2][i]))
            res[i].fill_(-1)
        for r in d_res:
            r.fill_(-1)
        torch.cuda.synchronize()
        if rep % 4 < 2:
            launch(cods[0], d_buf, d_res[0])  # direct scrubs on the current stream
            g.replay()                        # ... the graph between them
            launch(cods[0], d_buf, d_res[1])
        else:
            with torch.cuda.stream(other):
                g.replay()                    # the graph on another stream
            launch(cods[0], d_buf, d_res[0])  # while the current stream runs direct scrubs
            launch(cods[0], d_buf, d_res[1])
        torch.cuda.synchronize()
        for i in range(2):
            got = as_u64(res[i], S)
            if is_clean:
                assert not got.any(), (rep, i, got.tolist())
            else:
                assert np.array_equal(got, want[rep // 2 % 2][i]), (rep, i)
        for r in d_res:
            assert np.array_equal(as_u64(r, d_stripes), d_want), rep
    assert H.queue_stats(0)["graph_sets"] - g0 == 2
    del g


# ---- the fixed tile order of the product build ---------------------------------------

def test_fixed_tile_order_in_child_process():
    """Past 256 captured launches a process gets no more graph counter sets,
    and every launcher runs its fixed-order kernel.  That state is permanent,
    so a child process enters it (scrub_fixed_order_child.py: it reports
    graph_sets == 256 before and after capturing the graph it checks).  One
    child, started once."""
    child = subprocess.run([sys.executable, os.path.join(HERE, "scrub_fixed_order_child.py")], capture_output=True,
                           text=True, timeout=600)
    assert child.returncode == 0, (child.returncode, child.stdout[-2000:], child.stderr[-4000:])
    assert "graph_sets 0 -> 256 -> 256" in child.stdout and "fixed order ok" in child.stdout, child.stdout[-2000:]
