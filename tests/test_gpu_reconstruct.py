"""Reconstruction of any lost unit of a stripe, parity included, on the GPU:
hec_reconstruct_device (one pattern per batch) and
hec_reconstruct_device_mixed (one pattern per stripe; the gf_reconstruct_mixed
kernel and its per-run fallback).  The ground truth everywhere is the stripe
that was encoded -- random data plus the CPU oracle's parity -- compared as
exact bytes.  Most tests repair in place: the lost slots are scribbled over,
rebuilt into their own storage, and the WHOLE buffer must equal the expected
image, so a write to a present unit, to an unwanted slot or past cell_len
shows as well as a wrong byte."""
import ctypes
import itertools

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GARBAGE = 0xEE
# one 16-B chunk; a wave-tile (64 lanes x 4 chunks) + a tail; a 256-thread
# block's worth of wave-tiles + a wave-tile + a tail
CELLS = (16, 4096 + 16, 16384 + 4096 + 48)


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


def truth(k, m, S, cell):
    """The original stripes [S, k+m, cell] (computed once per shape, shared,
    read-only): random data and the oracle's parity rows applied to it."""
    key = (k, m, S, cell)
    if key not in _truth:
        rng = np.random.default_rng(7919 * k + 31 * m + S + cell)
        t = np.empty((S, k + m, cell), dtype=np.uint8)
        t[:, :k] = rng.integers(0, 256, size=(S, k, cell), dtype=np.uint8)
        # stripes are independent and the code is bytewise: one long shard per unit
        flat = [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)]
        par = O.matmul_shards(O.codec_matrix("rs", k, m)[k:], flat)
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        t.setflags(write=False)
        _truth[key] = t
    return _truth[key]


def patterns(n, lo, hi):
    return [lost for e in range(lo, hi + 1) for lost in itertools.combinations(range(n), e)]


def present_mask(n, lost):
    return ((1 << n) - 1) & ~sum(1 << i for i in lost)


def image(t, dev, pad=0):
    """Device copy of the stripes [S, n, cell + pad]; the pad bytes between
    cell_len and the stride hold GARBAGE."""
    S, n, cell = t.shape
    buf = torch.full((S, n, cell + pad), GARBAGE, dtype=torch.uint8, device=dev)
    buf[:, :, :cell] = torch.from_numpy(t.copy()).to(dev)
    return buf


def slots(buf):
    """(ptrs, strides) of the k+m unit slots of a [S, n, width] buffer."""
    S, n, width = buf.shape
    return [buf.data_ptr() + i * width for i in range(n)], [n * width] * n


def stream():
    return torch.cuda.current_stream().cuda_stream


def mixed_in_place(cod, t, losts, dev, wants=None, pad=0, workspace=None):
    """Scribbles over stripe s's units losts[s], repairs the batch in place
    with one mixed call and returns (buffer, expected): expected is the
    original with GARBAGE left in the pad and in lost units nobody wanted."""
    S, n, cell = t.shape
    expected = image(t, dev, pad)
    buf = expected.clone()
    for s, lost in enumerate(losts):
        for i in lost:
            buf[s, i] = GARBAGE
            if wants is not None and i not in wants[s]:
                expected[s, i] = GARBAGE
    ptrs, strides = slots(buf)
    masks = [present_mask(n, lost) for lost in losts]
    wmasks = None if wants is None else [sum(1 << i for i in w) for w in wants]
    if workspace is None:
        workspace = torch.empty(cod.reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    cod.reconstruct_device_mixed(ptrs, strides, ptrs, strides, masks, wmasks, cell, S, workspace.data_ptr(),
                                 workspace.numel(), stream())
    return buf, expected


# ---- one pattern per batch --------------------------------------------------

@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("cell", CELLS)
def test_uniform_rs63_every_pattern_in_place(dev, cell, S):
    """RS(6,3), all 129 patterns of 1..3 lost units, each on its own copy of
    the batch with the lost slots scribbled over and d_out[t] = d_shards[t]'s
    slot; one compare of all copies against the original at the end (S = 5:
    the tile group of 4 stripes plus a remainder)."""
    k, m, n = 6, 3, 9
    pats = patterns(n, 1, m)
    assert len(pats) == 129
    want = image(truth(k, m, S, cell), dev)
    bufs = want.unsqueeze(0).repeat(len(pats), 1, 1, 1)
    for p, lost in enumerate(pats):
        for i in lost:
            bufs[p, :, i] = GARBAGE
    for p, lost in enumerate(pats):
        ptrs, strides = slots(bufs[p])
        coder(k, m).reconstruct_device([None if i in lost else ptrs[i] for i in range(n)], strides, ptrs, strides,
                                       cell, S, stream=stream())
    torch.cuda.synchronize()
    bad = [pats[p] for p in range(len(pats)) if not torch.equal(bufs[p], want)]
    assert not bad, bad


def test_uniform_rs104_sample_separate_outputs(dev):
    """RS(10,4), a seeded sample of 40 patterns that includes 4 lost and all
    parity lost, into output buffers of their own: targets equal the original,
    every other out slot keeps its fill."""
    k, m, n, S, cell = 10, 4, 14, 3, 2048 + 32
    pats = patterns(n, 1, m)
    rng = np.random.default_rng(1040)
    picks = [pats[i] for i in rng.choice(len(pats), size=38, replace=False)] + [(10, 11, 12, 13), (0, 5, 9, 12)]
    src = image(truth(k, m, S, cell), dev)
    ptrs, strides = slots(src)
    outs = torch.full((len(picks),) + tuple(src.shape), 0xA5, dtype=torch.uint8, device=dev)
    for p, lost in enumerate(picks):
        optrs, ostrides = slots(outs[p])
        coder(k, m).reconstruct_device([None if i in lost else ptrs[i] for i in range(n)], strides, optrs, ostrides,
                                       cell, S, stream=stream())
    torch.cuda.synchronize()
    for p, lost in enumerate(picks):
        for i in range(n):
            if i in lost:
                assert torch.equal(outs[p, :, i], src[:, i]), (lost, i)
            else:
                assert bool((outs[p, :, i] == 0xA5).all()), (lost, i)


def test_uniform_byte_path_unaligned(dev):
    """cell_len 1000 on a base 1 byte off the 16-B grid: the byte-granular
    kernels, data and parity targets, in place."""
    k, m, n, S, cell = 6, 3, 9, 3, 1000
    t = truth(k, m, S, cell)
    for lost in [(0,), (8,), (2, 6), (1, 4, 7), (6, 7, 8)]:
        raw = torch.full((S * n * cell + 1,), GARBAGE, dtype=torch.uint8, device=dev)
        buf = raw[1:].view(S, n, cell)
        assert buf.data_ptr() % 16 == 1
        buf.copy_(torch.from_numpy(t.copy()).to(dev))
        for i in lost:
            buf[:, i] = GARBAGE
        ptrs, strides = slots(buf)
        coder(k, m).reconstruct_device([None if i in lost else ptrs[i] for i in range(n)], strides, ptrs, strides,
                                       cell, S, stream=stream())
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), t), lost
        assert int(raw[0]) == GARBAGE


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4), (3, 2)])
def test_uniform_all_parity_lost_is_encode(dev, k, m):
    """Every data unit present, all m parity units the targets: the rows are
    the coding matrix's parity rows, so this is hec_encode_device by another
    name -- the same bytes, and the oracle's parity.  Bytes cannot tell which
    kernel ran: that the encode kernels are chosen holds by construction, both
    calls reaching launch_gf_matmul through matmul_batch with identical
    coefficients, where rs_parity_matrix decides from the coefficients alone."""
    n, S, cell = k + m, 5, 16384 + 4096 + 48
    t = truth(k, m, S, cell)
    src = image(t, dev)
    ptrs, strides = slots(src)
    enc = torch.full((S, m, cell), 0xA5, dtype=torch.uint8, device=dev)
    rec = torch.full((S, n, cell), 0xA5, dtype=torch.uint8, device=dev)
    eptrs, estrides = H.stripe_layout_ptrs(enc, m)
    optrs, ostrides = slots(rec)
    coder(k, m).encode_device(ptrs[:k], strides[:k], eptrs, estrides, cell, S, stream())
    coder(k, m).reconstruct_device(ptrs[:k] + [None] * m, strides, optrs, ostrides, cell, S, stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(rec[:, k:], enc)
    assert torch.equal(enc, src[:, k:])
    assert bool((rec[:, :k] == 0xA5).all())


def test_uniform_want_subset_and_errors(dev):
    k, m, n, S, cell = 6, 3, 9, 2, 4096 + 16
    src = image(truth(k, m, S, cell), dev)
    ptrs, strides = slots(src)
    out = torch.full_like(src, 0xA5)
    optrs, ostrides = slots(out)
    lost = (1, 7)
    shards = [None if i in lost else ptrs[i] for i in range(n)]
    coder(k, m).reconstruct_device(shards, strides, optrs, ostrides, cell, S, want=[7], stream=stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:, 7], src[:, 7])
    out[:, 7] = 0xA5
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError):  # unit 0 is present
        coder(k, m).reconstruct_device(shards, strides, optrs, ostrides, cell, S, want=[0], stream=stream())
    # a NULL d_out at a target is refused before anything is launched
    no7 = [None if i == 7 else p for i, p in enumerate(optrs)]
    with pytest.raises(ValueError):
        coder(k, m).reconstruct_device(shards, strides, no7, ostrides, cell, S, stream=stream())
    coder(k, m).reconstruct_device(shards, strides, no7, ostrides, cell, S, want=[1], stream=stream())  # 7 not wanted
    torch.cuda.synchronize()
    assert torch.equal(out[:, 1], src[:, 1])
    out[:, 1] = 0xA5
    assert bool((out == 0xA5).all())
    with pytest.raises(H.ErasureCodingError):
        coder(k, m).reconstruct_device([None] * 4 + ptrs[4:], strides, optrs, ostrides, cell, S, stream=stream())
    # nothing wanted: no work, whatever is present
    coder(k, m).reconstruct_device([None] * 4 + ptrs[4:], strides, optrs, ostrides, cell, S, want=[], stream=stream())
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# ---- one pattern per stripe ---------------------------------------------------

@pytest.mark.parametrize("cell", CELLS)
def test_mixed_rs63_every_pattern(dev, cell):
    """RS(6,3), batches of 37 stripes cycling through the intact stripe and
    all 129 loss patterns (parity-only, data-only and data + parity losses in
    one launch), repaired in place."""
    k, m, S = 6, 3, 37
    pats = [()] + patterns(k + m, 1, m)
    t = truth(k, m, S, cell)
    runs = []
    for r in range((len(pats) + S - 1) // S):
        losts = [pats[(r * S + s) % len(pats)] for s in range(S)]
        runs.append((losts,) + mixed_in_place(coder(k, m), t, losts, dev))
    torch.cuda.synchronize()
    for losts, buf, expected in runs:
        bad = [losts[s] for s in range(S) if not torch.equal(buf[s], expected[s])]
        assert not bad, bad


def test_mixed_rs32(dev):
    k, m, S, cell = 3, 2, 19, 4096 + 16
    pats = [()] + patterns(k + m, 1, m)
    losts = [pats[s % len(pats)] for s in range(S)]
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)


def test_mixed_rs104(dev):
    k, m, S, cell = 10, 4, 23, 8192 + 2048 + 32  # U = 2: a 512-thread block tile + a wave-tile + a tail
    rng = np.random.default_rng(104)
    losts = [tuple(sorted(rng.choice(k + m, size=int(rng.integers(0, m + 1)), replace=False).tolist()))
             for _ in range(S)]
    losts[0], losts[1], losts[2] = (), (10, 11, 12, 13), (0, 9, 10, 13)
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)


KERNEL_SHAPES = [(k, r) for k in (2, 3, 6, 10) for r in (1, 2, 3, 4)]


@pytest.mark.parametrize("k,r", KERNEL_SHAPES, ids=[f"k{k}-r{r}" for k, r in KERNEL_SHAPES])
def test_mixed_every_kernel_shape(dev, k, r):
    """gf_reconstruct_mixed<K, R> at every (K, R) it is built for: RS(k,4), every
    stripe of the batch loses exactly r units (so the launch has r rows), data
    and parity among them; 528 B = 33 chunks in one wave-tile, 9232 B = a short
    last wave-tile."""
    m, S = 4, 4
    rng = np.random.default_rng(100 * k + r)
    for cell in (528, 9232):
        losts = [tuple(sorted(rng.choice(k + m, size=r, replace=False).tolist())) for _ in range(S)]
        losts[0] = tuple(range(r))                   # data units only (k = 2: data, then parity)
        losts[1] = tuple(range(k + m - r, k + m))    # parity units only
        buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev)
        torch.cuda.synchronize()
        assert torch.equal(buf, expected), (cell, losts)


def test_mixed_rs66_two_launches(dev):
    """RS(6,6) with 5 and 6 units lost per stripe: more than 4 target rows, so
    a second launch with row0 = 4 (the header's second word of target bytes)."""
    k, m, S, cell = 6, 6, 9, 4096 + 16
    rng = np.random.default_rng(66)
    losts = [tuple(sorted(rng.choice(k + m, size=5 + s % 2, replace=False).tolist())) for s in range(S)]
    losts[0], losts[1], losts[2] = (6, 7, 8, 9, 10, 11), (0, 1, 2, 3, 4, 5), (1, 11)
    ws = torch.empty(coder(k, m).reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)
    # the fused kernel ran, twice: the counters of launch groups 0 (rows 0..3)
    # and 1 (row0 = 4) were used, the other groups' never
    q = _queue_words(ws, S, k, [len(l) for l in sorted(set(losts))])
    assert bool(q[0, :, 0].any()) and bool(q[1, :, 0].any()), q[:2, :, 0].tolist()
    assert not bool(q[2:].any()) and not bool(q[:2, :, 1:].any())


def test_mixed_want_subset_keeps_fill(dev):
    """want masks that ask for fewer units than are missing, on slots 48 bytes
    wider than the cell: unwanted lost slots and the bytes between cell_len
    and the stride keep their fill."""
    k, m, S, cell = 6, 3, 13, 4096 + 16
    pats = patterns(k + m, 2, m)
    rng = np.random.default_rng(63)
    losts = [pats[i] for i in rng.choice(len(pats), size=S, replace=False)]
    wants = [lost[1:] if s % 3 else lost[:1] for s, lost in enumerate(losts)]
    wants[0] = ()          # nothing wanted: the stripe is skipped
    wants[1] = losts[1]    # everything
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev, wants=wants, pad=48)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)


def test_mixed_plans_past_resident_lds(dev):
    """RS(10,4), 160 stripes of 4 KiB cells, each with its own 4-unit loss:
    160 plans x (64 + 4 x 10 x 32) B = 220 KiB, more than the 156 KiB the
    kernel keeps resident -- one launch per run of stripes instead."""
    k, m, S, cell = 10, 4, 160, 4096
    pats = patterns(k + m, 4, 4)
    losts = pats[::len(pats) // S][:S]
    assert len(set(losts)) == S
    # the per-run route never touches the workspace: it keeps its fill
    ws = torch.full((coder(k, m).reconstruct_mixed_workspace_size(S),), 0x77, dtype=torch.uint8, device=dev)
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)
    assert bool((ws == 0x77).all())


def test_mixed_fallback_shapes(dev):
    """k = 4 has no fused kernel, and a stride off the 16-B grid cannot take
    it: both run per run of stripes, with the same results."""
    k, m, S, cell = 4, 2, 11, 4096 + 16
    pats = [()] + patterns(k + m, 1, m)
    losts = [pats[(3 * s) % len(pats)] for s in range(S)]
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev)
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)
    k, m = 6, 3
    pats = [()] + patterns(k + m, 1, m)
    losts = [pats[(7 * s) % len(pats)] for s in range(S)]
    buf, expected = mixed_in_place(coder(k, m), truth(k, m, S, cell), losts, dev, pad=7)  # stride 9 x 4119
    torch.cuda.synchronize()
    assert torch.equal(buf, expected)


def test_mixed_data_only_matches_decode_mixed(dev):
    """want = NULL on data-only losses is hec_decode_device_mixed's job: the
    same bytes in the same out slots."""
    k, m, S, cell = 6, 3, 21, 16384 + 4096 + 48
    pats = [()] + patterns(k, 1, m)  # data units only
    losts = [pats[(5 * s) % len(pats)] for s in range(S)]
    t = truth(k, m, S, cell)
    src = image(t, dev)
    for s, lost in enumerate(losts):
        for i in lost:
            src[s, i] = GARBAGE
    ptrs, strides = slots(src)
    masks = [present_mask(k + m, lost) for lost in losts]
    o_dec = torch.full((S, k, cell), 0xA5, dtype=torch.uint8, device=dev)
    o_rec = torch.full((S, k + m, cell), 0xA5, dtype=torch.uint8, device=dev)
    dptrs, dstrides = H.stripe_layout_ptrs(o_dec, k)
    rptrs, rstrides = slots(o_rec)
    ws_d = torch.empty(coder(k, m).decode_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(coder(k, m).reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    coder(k, m).decode_device_mixed(ptrs, strides, dptrs, dstrides, masks, cell, S, ws_d.data_ptr(), ws_d.numel(),
                                    stream())
    coder(k, m).reconstruct_device_mixed(ptrs, strides, rptrs, rstrides, masks, None, cell, S, ws_r.data_ptr(),
                                         ws_r.numel(), stream())
    torch.cuda.synchronize()
    assert torch.equal(o_rec[:, :k], o_dec)
    assert bool((o_rec[:, k:] == 0xA5).all())
    want = torch.from_numpy(t.copy()).to(dev)
    for s, lost in enumerate(losts):
        for i in lost:
            assert torch.equal(o_rec[s, i], want[s, i]), (s, i)


def test_mixed_not_enough_units_launches_nothing(dev):
    k, m, S, cell = 6, 3, 4, 4096
    t = truth(k, m, S, cell)
    losts = [(0,), (), (1, 2, 7, 8), (6,)]  # stripe 2 has k - 1 units
    with pytest.raises(H.ErasureCodingError):
        mixed_in_place(coder(k, m), t, losts, dev)
    # the same through explicit buffers: the outputs keep their fill
    src = image(t, dev)
    out = torch.full_like(src, 0xA5)
    ptrs, strides = slots(src)
    optrs, ostrides = slots(out)
    ws = torch.empty(coder(k, m).reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    rc = H.lib.hec_reconstruct_device_mixed(coder(k, m).handle, H._pp(ptrs), H._sp(strides), H._pp(optrs),
                                            H._sp(ostrides), (ctypes.c_uint64 * S)(*[present_mask(9, l) for l in losts]),
                                            None, cell, S, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                            ctypes.c_void_p(stream()))
    assert rc == H.HEC_ERR_NOT_ENOUGH_SHARDS
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # a want bit on a present unit
    with pytest.raises(ValueError):
        mixed_in_place(coder(k, m), t, [(0,), (), (1,), (6,)], dev, wants=[(0,), (), (1, 3), (6,)])
    # a target without an output slot
    optrs[6] = None
    with pytest.raises(ValueError):
        coder(k, m).reconstruct_device_mixed(ptrs, strides, optrs, ostrides, [present_mask(9, (6,))] * S, None, cell,
                                             S, ws.data_ptr(), ws.numel(), stream())
    # ... which is fine when no stripe targets that unit
    coder(k, m).reconstruct_device_mixed(ptrs, strides, optrs, ostrides, [present_mask(9, (2,))] * S, None, cell, S,
                                         ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    assert torch.equal(out[:, 2], src[:, 2])


def test_host_only_coder_has_no_device_calls(dev):
    c = H.Coder(6, 3, H.HEC_DEVICE_HOST)
    buf = torch.zeros((2, 9, 64), dtype=torch.uint8, device=dev)
    ptrs, strides = slots(buf)
    ws = torch.empty(c.reconstruct_mixed_workspace_size(2), dtype=torch.uint8, device=dev)
    with pytest.raises(H.DeviceError):
        c.reconstruct_device([None] + ptrs[1:], strides, ptrs, strides, 64, 2)
    with pytest.raises(H.DeviceError):
        c.reconstruct_device_mixed(ptrs, strides, ptrs, strides, [0x1FE, 0x1FF], None, 64, 2, ws.data_ptr(),
                                   ws.numel())
    c.close()


def test_tensor_helper_repairs_in_place(dev):
    k, m, S, cell = 6, 3, 8, 4096 + 16
    t = truth(k, m, S, cell)
    cells = image(t, dev)
    want = cells.clone()
    losts = [(s % 9,) for s in range(S)]  # one lost unit per stripe: a dead node's block groups
    for s, lost in enumerate(losts):
        cells[s, lost[0]] = GARBAGE
    ws = H.reconstruct_batch_mixed(coder(k, m), cells, [present_mask(9, l) for l in losts])
    torch.cuda.synchronize()
    assert torch.equal(cells, want)
    cells[3, 0] = GARBAGE
    cells[3, 8] = GARBAGE
    H.reconstruct_batch_mixed(coder(k, m), cells, [0x1FF] * 3 + [present_mask(9, (0, 8))] + [0x1FF] * 4,
                              want_masks=[0] * 3 + [1 << 8] + [0] * 4, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(cells[3, 8], want[3, 8]) and bool((cells[3, 0] == GARBAGE).all())


# ---- tile counters ------------------------------------------------------------

def _queue_words(ws, S, k, plans):
    """The launch counters of a mixed call's workspace: [plan offsets][plan
    blob][counters], each part 256-B aligned; `plans` = target counts of the
    distinct (present, want) pairs."""
    def up(v):
        return (v + 255) & ~255
    pos = up(up(4 * S) + sum(64 + e * k * 32 for e in plans))
    return ws[pos:pos + 16 * 8 * 256].view(torch.int32).view(16, 8, 64)


@pytest.mark.parametrize("k,m", [(6, 3), (3, 2)])
def test_mixed_back_to_back_tile_counters(dev, k, m):
    """Two mixed calls back to back on one stream, each with a workspace of
    its own (the launch deals its wave-tiles from counters the workspace
    upload zeroes): both correct, the first launch group's counters were
    used, the others never touched, and no stream counter set was taken."""
    S, cell = 16, 16384 + 4096 + 48
    t = truth(k, m, S, cell)
    pats = patterns(k + m, 1, m)
    before = H.queue_stats(0)["streams"]
    runs = []
    for call in range(2):
        losts = [pats[(11 * call + 5 * s) % len(pats)] for s in range(S)]
        ws = torch.empty(coder(k, m).reconstruct_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        runs.append((losts, ws) + mixed_in_place(coder(k, m), t, losts, dev, workspace=ws))
    torch.cuda.synchronize()
    assert H.queue_stats(0)["streams"] == before
    for losts, ws, buf, expected in runs:
        assert torch.equal(buf, expected)
        q = _queue_words(ws, S, k, [len(l) for l in sorted(set(losts))])
        used = q[0, :, 0]
        tiles = S * -(-(cell // 16) // 256)  # wave-tiles of 64 lanes x 4 chunks
        rounds = 1 if k >= 6 else 4
        # every wave ends on a fetch past the end; the fetches before it hand out all the tiles
        assert int(used.sum()) * rounds >= tiles and bool((used > 0).all()), used.tolist()
        assert not bool(q[1:].any()) and not bool(q[0, :, 1:].any())
