"""Degraded scrub on the GPU (hec_scrub_device_mixed: one presence mask per
stripe).  Expected results come from degraded_scrub_ref (rebuild-and-compare
over the oracle's matrix routines, not the kernels' syndromes and minors),
evaluated for every stripe of every batch; the WHOLE result array is compared,
exactly.  Every result buffer is handed in filled with 0xFF (the call zeroes it
itself) and the slots a stripe lacks are filled with random garbage, so a
kernel that reads them shows.

Which kernel each test reaches (ScrubMixedFn in csrc/ec_scrub_mixed.hip builds
gf_scrub_mixed<K, M, U, BS, WQ> for K in {2, 3, 6, 10} x M in {1, 2, 3, 4}: WQ > 0
with the batch's plans resident in LDS, WQ == 0 for the uniform-plan launches
of a batch whose plans overflow it; M is the largest e of the batch):

  test                                    kernels
  --------------------------------------  -----------------------------------------
  test_all_present_equals_scrub_device    gf_scrub_mixed<K, M, WQ > 0>, all 16 (K, M)
                                            with rs (e == m), M == 1 again with xor,
                                            rs-legacy at (3,2), (6,3), (10,4)
  test_every_pattern                      gf_scrub_mixed<6,3 / 10,4 / 3,2 / 2,1,
                                            WQ > 0>, every e <= M in one launch,
                                            unchecked stripes (kNoPlan) among them;
                                            cells of one chunk, one wave-tile, three
                                            wave-tiles + 48 bytes
  test_mixed_e_in_one_launch              gf_scrub_mixed<10,4> and <6,4>, WQ > 0:
                                            e = 4, 3, 2, 1, 0 interleaved (the row
                                            skip, M above a stripe's e)
  test_more_plans_than_lds                gf_scrub_mixed<10, 1..4, WQ == 0>, one
                                            uniform-plan launch per stripe (470
                                            masks); <10,4, WQ > 0> for the part
                                            that fits
  test_generic_kernel, test_xor_5_1       gf_scrub_mixed_bytes: k = 5, 4, 32, up to
                                            16 extras, odd cells, a base off the
                                            grid, units numbered 32 and up
  test_more_tiles_than_waves              gf_scrub_mixed<6,3> and <10,4>, WQ > 0,
                                            every wave through the tile loop twice
  test_stripe_stride_past_4gib            gf_scrub_mixed<6,3, WQ > 0> and
                                            gf_scrub_mixed_bytes, stripe offsets of
                                            2^32 and more
  test_two_streams_at_once                gf_scrub_mixed<6,3, WQ > 0>, two
                                            workspaces (two sets of counters)
  test_degraded_loop                      gf_scrub_mixed<6,2, WQ > 0>, then
                                            gf_reconstruct_mixed and gf_scrub
  test_arguments_queue_nothing            none: every call is refused
"""
import ctypes
import itertools

import numpy as np
import pytest

import degraded_scrub_ref as R
import hdfs_native_ec as H
from test_gpu_scrub import (S, TILE, _ref_batch, as_u64, assorted_corruptions, coder, consistent_stripes, dev,  # noqa: F401
                            prefilled, scrub, stream, truth)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def with_garbage(cells, masks, seed=99):
    """A copy of cells [stripes, k+m, cell] with every slot its stripe's mask
    lacks overwritten by random bytes."""
    out = np.array(cells)
    rng = np.random.default_rng(seed)
    n, cell = out.shape[1], out.shape[2]
    for st, mask in enumerate(masks):
        for t in range(n):
            if not (mask >> t) & 1:
                out[st, t] = rng.integers(0, 256, size=cell, dtype=np.uint8)
    return out


def launch(cod, buf, masks, res, ws, st=None):
    """hec_scrub_device_mixed over a device tensor [stripes, k+m, cell]; asynchronous."""
    n, cell = buf.shape[1], buf.shape[2]
    ptrs, strides = H.stripe_layout_ptrs(buf, n)
    cod.scrub_device_mixed(ptrs, strides, masks, cell, buf.shape[0], res.data_ptr(), ws.data_ptr(), ws.numel(),
                           stream() if st is None else st.cuda_stream)


def workspace(cod, stripes, dev):
    return torch.full((cod.scrub_mixed_workspace_size(stripes),), 0xA5, dtype=torch.uint8, device=dev)


def scrub_mixed(cod, cells, masks, dev):
    """One call over a numpy image (missing slots garbage) into a 0xFF-filled
    buffer, with a workspace of exactly the size the coder asks for."""
    buf = torch.from_numpy(with_garbage(cells, masks)).to(dev)
    res = prefilled(len(masks), dev)
    launch(cod, buf, masks, res, workspace(cod, len(masks), dev))
    torch.cuda.synchronize()
    return as_u64(res, len(masks))


def lose(n, lost):
    mask = (1 << n) - 1
    for t in lost:
        mask &= ~(1 << int(t))
    return mask


KINDS = ("survivor-byte", "extra-byte", "first-and-last", "whole-unit", "two-units")


def corrupt(cells, st, k, mask, kind, rng):
    """One corruption of stripe st (in place), among its present units."""
    n, cell = cells.shape[1], cells.shape[2]
    pres = R.present_units(n, mask)
    surv, extras = pres[:k], pres[k:] or pres
    flip = lambda: int(rng.integers(1, 256))  # noqa: E731
    if kind == "survivor-byte":
        cells[st, surv[int(rng.integers(0, len(surv)))], int(rng.integers(0, cell))] ^= flip()
    elif kind == "extra-byte":
        cells[st, extras[int(rng.integers(0, len(extras)))], int(rng.integers(0, cell))] ^= flip()
    elif kind == "first-and-last":
        t = pres[int(rng.integers(0, len(pres)))]
        cells[st, t, 0] ^= flip()
        cells[st, t, cell - 1] ^= flip() if cell > 1 else 0
    elif kind == "whole-unit":
        cells[st, pres[int(rng.integers(0, len(pres)))]] = rng.integers(0, 256, size=cell, dtype=np.uint8)
    else:
        a, b = (int(t) for t in rng.choice(pres, size=2, replace=len(pres) < 2))
        cells[st, a, int(rng.integers(0, cell))] ^= flip()
        cells[st, b, int(rng.integers(0, cell))] ^= flip()


def check(cod, codec, k, m, cells, masks, dev):
    want = R.ref_batch(codec, k, m, cells, masks)
    got = scrub_mixed(cod, cells, masks, dev)
    diff = np.nonzero((got != want).any(axis=1))[0]
    assert len(diff) == 0, (diff.tolist()[:8], [hex(masks[i]) for i in diff[:8]], got[diff[:8]].tolist(),
                            want[diff[:8]].tolist())
    return want


# ---- 1. all present: the words of hec_scrub_device --------------------------------

ALL_PRESENT = [("rs", k, m) for k in (2, 3, 6, 10) for m in (1, 2, 3, 4)]
ALL_PRESENT += [("xor", k, 1) for k in (2, 3, 6, 10)] + [("rs-legacy", 3, 2), ("rs-legacy", 6, 3), ("rs-legacy", 10, 4)]


@pytest.mark.parametrize("codec,k,m", ALL_PRESENT, ids=[f"{c}-{k}-{m}" for c, k, m in ALL_PRESENT])
def test_all_present_equals_scrub_device(dev, codec, k, m):
    cell = TILE[k] + 16
    cod = coder(k, m, codec)
    full = [lose(k + m, ())] * S
    cells, _ = assorted_corruptions(codec, k, m, cell, TILE[k])
    uniform = scrub(cod, cells, dev)
    assert uniform[:, 1].any()
    assert np.array_equal(scrub_mixed(cod, cells, full, dev), uniform)
    assert np.array_equal(uniform, R.ref_batch(codec, k, m, cells, full))  # the two references agree
    assert not scrub_mixed(cod, truth(codec, k, m, S, cell), full, dev).any()


# ---- 2. every pattern -----------------------------------------------------------------

def pattern_masks(k, m):
    """Every mask that can be checked (fewer than m lost) for the small
    shapes, all single losses and 40 sampled double and triple losses for
    (10,4); then masks with m and m + 1 lost (unchecked); shuffled."""
    n = k + m
    rng = np.random.default_rng(1000 * k + m)
    if (k, m) == (10, 4):
        losses = [()] + [(t,) for t in range(n)]
        for r in (2, 3):
            combos = list(itertools.combinations(range(n), r))
            losses += [combos[i] for i in rng.choice(len(combos), size=20, replace=False)]
    else:
        losses = [c for r in range(m) for c in itertools.combinations(range(n), r)]
    for r in (m, m + 1):
        combos = list(itertools.combinations(range(n), r))
        losses += [combos[i] for i in rng.choice(len(combos), size=min(3, len(combos)), replace=False)]
    masks = [lose(n, c) for c in losses]
    return [masks[i] for i in rng.permutation(len(masks))]


PATTERNS = [("rs", 6, 3, c) for c in (16, 4096, 12336)] + [("rs", 10, 4, c) for c in (16, 2048, 6160)]
PATTERNS += [("rs", 3, 2, c) for c in (16, 4096, 12336)] + [("rs", 2, 1, c) for c in (16, 4096, 12336)]


@pytest.mark.parametrize("codec,k,m,cell", PATTERNS, ids=[f"{c}-{k}-{m}-{cell}" for c, k, m, cell in PATTERNS])
def test_every_pattern(dev, codec, k, m, cell):
    base = pattern_masks(k, m)
    if (k, m) == (6, 3):
        assert sum(bin(x).count("1") >= k + m - 2 for x in base) == 46
    masks = base * len(KINDS)  # every mask meets every kind of corruption
    cod = coder(k, m, codec)
    clean = truth(codec, k, m, len(masks), cell)
    assert not scrub_mixed(cod, clean, masks, dev).any()
    cells = clean.copy()
    rng = np.random.default_rng(cell + 7 * k)
    for st, mask in enumerate(masks):
        corrupt(cells, st, k, mask, KINDS[st // len(base)], rng)
    want = check(cod, codec, k, m, cells, masks, dev)
    checkable = np.array([bin(x).count("1") > k for x in masks])
    assert want[checkable, 1].all() and not want[~checkable].any()
    n = k + m
    for st in np.nonzero(checkable)[0]:
        missing = ~masks[st] & ((1 << n) - 1)
        assert int(want[st, 0]) & missing == missing  # a missing unit is never the culprit


# ---- 3. mixed e in one launch ---------------------------------------------------------

@pytest.mark.parametrize("k,m", [(10, 4), (6, 4)], ids=["rs-10-4", "rs-6-4"])
def test_mixed_e_in_one_launch(dev, k, m):
    n, cell, stripes = k + m, 2 * TILE[k] + 16, 45
    rng = np.random.default_rng(k)
    masks = [lose(n, rng.choice(n, size=st % 5, replace=False)) for st in range(stripes)]  # e = 4, 3, 2, 1, 0, 4, ...
    assert [bin(x).count("1") - k for x in masks[:5]] == [4, 3, 2, 1, 0]
    cod = coder(k, m)
    clean = truth("rs", k, m, stripes, cell)
    assert not scrub_mixed(cod, clean, masks, dev).any()
    cells = clean.copy()
    for st in range(stripes):
        if st % 7 != 6:
            corrupt(cells, st, k, masks[st], KINDS[st % len(KINDS)], rng)
    want = check(cod, "rs", k, m, cells, masks, dev)
    hit = [st for st in range(stripes) if st % 7 != 6 and st % 5 != 4]  # corrupted, and with something to check against
    assert np.nonzero(want[:, 1])[0].tolist() == hit and not want[4::5].any()


# ---- 4. more plans than the LDS holds -------------------------------------------------

def test_more_plans_than_lds(dev):
    """All 470 masks of (10,4) that can be checked, one per stripe: 214 KiB of
    plans against 156 KiB of resident LDS, so every stripe is a uniform-plan
    launch.  The first 200 stripes alone fit and run the resident kernel: the
    same words."""
    codec, k, m, cell = "rs", 10, 4, 2064
    n = k + m
    masks = [lose(n, c) for r in range(m) for c in itertools.combinations(range(n), r)]
    assert len(masks) == len(set(masks)) == 470
    rng = np.random.default_rng(470)
    masks = [masks[i] for i in rng.permutation(470)]
    blob = sum(64 + (bin(x).count("1") - k) * k * 32 for x in masks)
    assert blob > 156 << 10 > sum(64 + (bin(x).count("1") - k) * k * 32 for x in masks[:200]) + 4 * 200
    cod = coder(k, m)
    clean = truth(codec, k, m, 470, cell)
    assert not scrub_mixed(cod, clean, masks, dev).any()
    cells = clean.copy()
    for st in range(470):
        if st % 3 != 2:
            corrupt(cells, st, k, masks[st], KINDS[st % len(KINDS)], rng)
    want = check(cod, codec, k, m, cells, masks, dev)
    assert np.array_equal(scrub_mixed(cod, cells[:200], masks[:200], dev), want[:200])


# ---- 5. the byte-granular kernel ------------------------------------------------------

GENERIC = [("rs", 5, 3, 2, 1000), ("rs", 5, 3, 2, 37), ("rs", 4, 8, 7, 1000), ("rs", 4, 8, 7, 37),
           ("rs", 32, 16, 5, 1000), ("rs", 32, 16, 5, 37)]


@pytest.mark.parametrize("codec,k,m,max_lost,cell", GENERIC, ids=[f"{c}-{k}-{m}-{cell}" for c, k, m, _, cell in GENERIC])
def test_generic_kernel(dev, codec, k, m, max_lost, cell):
    n = k + m
    rng = np.random.default_rng(n + cell)
    if k == 32:
        # two masks (the reference inverts a 32 x 32 matrix per unit and mask):
        # nothing lost, and five units lost on both sides of bit 32
        kinds = [(), (3, 30, 33, 40, 47)]
        stripes = 8
    else:
        kinds = [tuple(rng.choice(n, size=r, replace=False)) for r in range(max_lost + 1) for _ in range(3)]
        kinds += [tuple(rng.choice(n, size=m, replace=False))]  # unchecked
        stripes = 2 * len(kinds)
    masks = [lose(n, kinds[st % len(kinds)]) for st in range(stripes)]
    cod = coder(k, m, codec)
    clean = truth(codec, k, m, stripes, cell)
    assert not scrub_mixed(cod, clean, masks, dev).any()
    cells = clean.copy()
    for st in range(stripes):
        if st != 1:
            corrupt(cells, st, k, masks[st], KINDS[st % len(KINDS)] if k != 32 else KINDS[st % 3], rng)
    want = check(cod, codec, k, m, cells, masks, dev)
    if k == 32:
        assert int(np.bitwise_or.reduce(want[:, 0])) >> 32 != 0  # the high half of the words
    # every base one byte off the 16-byte grid
    image = with_garbage(cells, masks)
    flat = torch.full((image.size + 16,), 0xEE, dtype=torch.uint8, device=dev)
    flat[1:1 + image.size] = torch.from_numpy(image.reshape(-1)).to(dev)
    res = prefilled(stripes, dev)
    ws = workspace(cod, stripes, dev)
    cod.scrub_device_mixed([flat.data_ptr() + 1 + i * cell for i in range(n)], [n * cell] * n, masks, cell, stripes,
                           res.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(as_u64(res, stripes), want)


def test_xor_5_1(dev):
    codec, k, m, cell = "xor", 5, 1, 1000
    n = k + m
    cells = truth(codec, k, m, 12, cell).copy()
    for st in range(12):
        cells[st, st % n, (st * 97) % cell] ^= 1 + st
    cod = coder(k, m, codec)
    full = [lose(n, ())] * 12
    want = check(cod, codec, k, m, cells, full, dev)
    assert want[:, 1].tolist() == [1] * 12 and not want[:, 0].any()  # one check cannot locate
    assert np.array_equal(want, _ref_batch(codec, k, m, cells))
    # any loss leaves k units: unchecked, and with the results still zeroed
    assert not scrub_mixed(cod, cells, [lose(n, (st % n,)) for st in range(12)], dev).any()


# ---- 6. tile loop and addressing ------------------------------------------------------

def node_loss_masks(n, stripes, rng):
    """One unit missing per stripe, the index uniform over the k+m units."""
    return [lose(n, (int(t),)) for t in rng.integers(0, n, size=stripes)]


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)], ids=["rs-6-3", "rs-10-4"])
def test_more_tiles_than_waves(dev, k, m):
    """4 wave-tiles per stripe and more than twice as many tiles as the launch
    keeps waves resident (one block per CU): every wave fetches from its
    counter again after its first tile, and the last fetches land past the end."""
    waves = torch.cuda.get_device_properties(0).multi_processor_count * (8 if k == 10 else 4)
    stripes, cell = -(-2 * waves // 4) + 1, 3 * TILE[k] + 16
    n = k + m
    rng = np.random.default_rng(3 * k)
    masks = node_loss_masks(n, stripes, rng)
    cells = consistent_stripes("rs", k, m, stripes, cell)
    cod = coder(k, m)
    assert not scrub_mixed(cod, cells, masks, dev).any()
    hit = sorted({0, 3, 4, 5, stripes // 2, stripes - 2, stripes - 1} | set(rng.choice(stripes, size=14).tolist()))
    for x, st in enumerate(hit):
        corrupt(cells, st, k, masks[st], KINDS[x % len(KINDS)], rng)
    want = check(cod, "rs", k, m, cells, masks, dev)
    assert np.nonzero(want[:, 1])[0].tolist() == hit


def test_stripe_stride_past_4gib(dev):
    """17 stripes 2^28 bytes apart, as test_gpu_scrub_variants.py: stripe 16
    begins 2^32 bytes after stripe 0.  Once with 16-byte aligned bases (the
    register kernel), once with every base one byte on (the byte kernel)."""
    codec, k, m, cell = "rs", 6, 3, 4112
    n, stripes, stride = k + m, 17, 1 << 28
    masks = [lose(n, (st % n,)) for st in range(stripes)]
    masks[15] = lose(n, ())
    cells = truth(codec, k, m, stripes, cell).copy()
    cells[0, 2, 5] ^= 0x01
    cells[15, 7, cell - 1] ^= 0x40
    cells[16, 0, 0] ^= 0x80
    cells[16, 0, 4100] ^= 0x03
    want = R.ref_batch(codec, k, m, cells, masks)
    assert want[:, 1].tolist() == [1] + [0] * 14 + [1, 2]
    assert H.scrub_verdict(int(want[16, 0]), 2, n) == (H.HEC_SCRUB_LOCATED, 0)
    big = torch.empty(16 * stride + n * cell + 32, dtype=torch.uint8, device=dev)  # only the cells are written
    image = torch.from_numpy(with_garbage(cells, masks)).to(dev)
    cod = coder(k, m)
    ws = workspace(cod, stripes, dev)
    for off in (0, 1):
        base = big.data_ptr() + off
        assert base % 16 == off and 16 * stride >= 1 << 32
        for st in range(stripes):
            big[st * stride + off:st * stride + off + n * cell].copy_(image[st].reshape(-1))
        res = prefilled(stripes, dev)
        cod.scrub_device_mixed([base + i * cell for i in range(n)], [stride] * n, masks, cell, stripes,
                               res.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        torch.cuda.synchronize()
        got = as_u64(res, stripes)
        assert np.array_equal(got, want), (off, got.tolist(), want.tolist())
    del big


def test_two_streams_at_once(dev):
    """Two streams share one (6,3) coder, each with its own workspace, image
    and masks; both launched before one synchronize, three rounds."""
    codec, k, m = "rs", 6, 3
    n, stripes, cell = k + m, 149, 3 * TILE[k] + 16
    cod = coder(k, m)
    clean = consistent_stripes(codec, k, m, stripes, cell)
    bufs, masks, want = [], [], []
    for i in range(2):
        rng = np.random.default_rng(800 + i)
        mk = node_loss_masks(n, stripes, rng)
        cells = clean.copy()
        for x, st in enumerate(rng.choice(stripes, size=25, replace=False)):
            corrupt(cells, int(st), k, mk[st], KINDS[x % len(KINDS)], rng)
        want.append(R.ref_batch(codec, k, m, cells, mk))
        bufs.append(torch.from_numpy(with_garbage(cells, mk, seed=i)).to(dev))
        masks.append(mk)
    assert not np.array_equal(want[0], want[1])
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    wss = [workspace(cod, stripes, dev) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(3):
        res = [prefilled(stripes, dev) for _ in range(2)]
        torch.cuda.synchronize()
        for i in range(2):
            launch(cod, bufs[i], masks[i], res[i], wss[i], streams[i])
        torch.cuda.synchronize()
        for i in range(2):
            assert np.array_equal(as_u64(res[i], stripes), want[i]), i


# ---- 7. the degraded loop -------------------------------------------------------------

def test_degraded_loop(dev):
    """A node loss: one unit missing per stripe, one stripe in ten with a
    corrupt survivor as well.  Scrub with the masks, clear each located unit
    from its mask, rebuild both units in place, scrub the whole stripes."""
    codec, k, m, cell = "rs", 6, 3, 4112
    n, stripes = k + m, 120
    rng = np.random.default_rng(77)
    masks = node_loss_masks(n, stripes, rng)
    orig = truth(codec, k, m, stripes, cell)
    cells = orig.copy()
    hit = {}
    for st in rng.choice(stripes, size=stripes // 10, replace=False):
        pres = R.present_units(n, masks[st])
        hit[int(st)] = pres[int(rng.integers(0, len(pres)))]
        if len(hit) % 2:
            cells[st, hit[int(st)]] = rng.integers(0, 256, size=cell, dtype=np.uint8)
        else:
            cells[st, hit[int(st)], rng.choice(cell, size=5, replace=False)] ^= 0x5A
    cod = coder(k, m)
    buf = torch.from_numpy(with_garbage(cells, masks)).to(dev)
    first = H.scrub_batch_mixed(cod, buf, masks)
    torch.cuda.synchronize()
    assert first.dtype == torch.int64 and tuple(first.shape) == (stripes, 2)
    assert np.array_equal(as_u64(first, stripes), R.ref_batch(codec, k, m, cells, masks))
    repaired = []
    for st, (ruled, bad) in enumerate(as_u64(first, stripes).tolist()):
        verdict, unit = H.scrub_verdict(ruled, bad, n)
        if st in hit:
            assert (verdict, unit) == (H.HEC_SCRUB_LOCATED, hit[st]), st  # e == 2 locates one corrupt unit
            repaired.append(masks[st] & ~(1 << unit))
        else:
            assert verdict == H.HEC_SCRUB_CLEAN, st
            repaired.append(masks[st])
    H.reconstruct_batch_mixed(cod, buf, repaired)  # every unit outside the mask: the lost one and the located one
    second = H.scrub_batch(cod, buf)
    torch.cuda.synchronize()
    assert not as_u64(second, stripes).any()
    assert torch.equal(buf.cpu(), torch.from_numpy(orig.copy()))


# ---- 8. arguments ---------------------------------------------------------------------

def test_arguments_queue_nothing(dev):
    codec, k, m, cell = "rs", 6, 3, 4112
    n = k + m
    buf = torch.from_numpy(truth(codec, k, m, S, cell).copy()).to(dev)
    buf[3, 2, 9] ^= 1
    ptrs, strides = H.stripe_layout_ptrs(buf, n)
    res = prefilled(S, dev)
    cod = coder(k, m)
    lib = cod._lib
    need = cod.scrub_mixed_workspace_size(S)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    masks = (ctypes.c_uint64 * S)(*[lose(n, (st % n,)) for st in range(S)])

    def call(h, p, st, pm, cell_len, results, w, wbytes, count=S):
        return lib.hec_scrub_device_mixed(h, None if p is None else H._pp(p), None if st is None else H._sp(st), pm,
                                          cell_len, count, ctypes.c_void_p(results), ctypes.c_void_p(w), wbytes,
                                          ctypes.c_void_p(stream()))

    ok = (cod.handle, ptrs, strides, masks, cell, res.data_ptr(), ws.data_ptr(), need)
    bad = H.HEC_ERR_INVALID_ARG
    assert call(None, *ok[1:]) == bad
    assert call(cod.handle, None, *ok[2:]) == bad
    assert call(*ok[:2], None, *ok[3:]) == bad
    assert call(*ok[:3], None, *ok[4:]) == bad
    for t in (0, k, n - 1):
        assert call(cod.handle, [0 if i == t else p for i, p in enumerate(ptrs)], *ok[2:]) == bad
    assert call(*ok[:4], 0, *ok[5:]) == bad
    assert call(*ok[:5], 0, *ok[6:]) == bad
    assert call(*ok[:5], res.data_ptr() + 4, *ok[6:]) == bad  # 8-byte alignment
    assert call(*ok[:6], 0, need) == bad  # no workspace
    assert call(*ok[:7], need - 1) == bad  # one byte short
    assert call(*ok[:6], ws.data_ptr() + 1, need) == bad  # misaligned
    host = H.Coder(k, m, H.HEC_DEVICE_HOST)
    assert call(host.handle, *ok[1:]) == H.HEC_ERR_DEVICE
    with pytest.raises(H.DeviceError):
        host.scrub_device_mixed(ptrs, strides, list(masks), cell, S, res.data_ptr(), ws.data_ptr(), need, stream())
    host.close()
    assert call(*ok, count=0) == H.HEC_OK  # no stripe: nothing queued
    torch.cuda.synchronize()
    assert (res == -1).all()  # the pre-fill is untouched: nothing was queued
    # no checkable stripe: HEC_OK without a workspace, and the results are zeroed
    none = (ctypes.c_uint64 * S)(*[lose(n, (0, 4, 8))] * S)
    assert call(*ok[:3], none, cell, res.data_ptr(), 0, 0) == H.HEC_OK
    torch.cuda.synchronize()
    assert not as_u64(res, S).any()
    # and the call the refusals were measured against goes through
    res.fill_(-1)
    assert call(*ok) == H.HEC_OK
    torch.cuda.synchronize()
    got = as_u64(res, S)
    assert got[:, 1].tolist() == [1 if st == 3 else 0 for st in range(S)]
    assert H.scrub_verdict(int(got[3, 0]), 1, n) == (H.HEC_SCRUB_LOCATED, 2)
