"""Verified scrub on the GPU: hec_scrub_crc_device (every unit present) and
hec_scrub_crc_device_mixed (one presence mask per stripe) -- the fused
gf_scrub_crc kernel and the composed route.

Ground truth is never the code under test.  The parity results come from
degraded_scrub_ref.ref_batch (rebuilds and comparisons over the oracle's matrix
routines) on the cells actually uploaded; the flags come from a numpy
comparison of the C oracle's chunk sums (orc_chunk_checksum) of the cells
actually uploaded against the expected sums actually uploaded.  Whole arrays
are compared exactly.

Every buffer carries sentinels: d_results arrives filled with 0xFF, missing
slots hold random bytes in the cells and 0xA5 in every byte of their sums, the
padding between cell_len and the stride holds 0xEE.  After every call the cell
buffer and the expected-sums buffer must be byte-identical to what was
uploaded."""
import ctypes

import numpy as np
import pytest

import degraded_scrub_ref as R
import ec_oracle as O
import hdfs_native_ec as H
import test_gpu_reconstruct_crc as RC
from test_gpu_scrub import coder, dev, prefilled, as_u64  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GARBAGE = 0xEE
SENT = 0xA5
CELLS = RC.CELLS  # (16, 528, 9232, 50192)
C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
PAD = 16  # bytes between cell_len and the stride


def full(n):
    return (1 << n) - 1


def lose(n, lost):
    return full(n) & ~sum(1 << i for i in lost)


class Batch:
    """One call's device buffers, what was uploaded, and the expected outputs.

    cells [S, n, cell] and sums [S, n, nck, 4] are numpy images, already
    corrupted as the case wants; masks (None: every unit present) say which
    slots exist.  preset = [(stripe, unit)] flags set before the call."""

    def __init__(self, codec, k, m, cells, sums, dev, masks=None, preset=(), base_off=0, bpc=512, ctype=C32C,
                 seed=1, raw=False):
        S, n, cell = cells.shape
        if raw:  # whole images as they are (padding and missing slots included): nothing is filled in
            cell -= PAD
        self.codec, self.k, self.m, self.S, self.n, self.cell = codec, k, m, S, n, cell
        self.bpc, self.ctype = bpc, ctype
        self.masks = [full(n)] * S if masks is None else [int(x) for x in masks]
        self.mixed_form = masks is not None
        present = np.array([[(mk >> u) & 1 for u in range(n)] for mk in self.masks], dtype=bool)
        rng = np.random.default_rng(seed)
        if raw:
            img, simg = np.array(cells, dtype=np.uint8), np.array(sums, dtype=np.uint8)
        else:
            img = np.full((S, n, cell + PAD), GARBAGE, dtype=np.uint8)
            img[:, :, :cell] = cells
            junk = rng.integers(0, 256, size=(S, n, cell), dtype=np.uint8)
            img[:, :, :cell][~present] = junk[~present]
            simg = np.array(sums, dtype=np.uint8)
            simg[~present] = SENT
        self.h_cells, self.h_sums, self.present = img, simg, present
        flat = torch.full((img.size + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = flat[base_off:].view(S, n, cell + PAD)
        self.cells.copy_(torch.from_numpy(img).to(dev))
        self.exp = torch.from_numpy(simg).to(dev)
        assert self.exp.data_ptr() % 4 == 0
        self.res = prefilled(S, dev)
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        h_bad = np.zeros((S, n), dtype=np.uint8)
        for (s, u) in preset:
            self.bad[s, u] = 1
            h_bad[s, u] = 1
        # ground truth: the oracle's sums of the uploaded cells against the uploaded sums ...
        actual = RC.chunk_sums(img[:, :, :cell], bpc, ctype)
        mismatch = (actual != simg).any(axis=(2, 3)) & present
        self.want_bad = h_bad | mismatch.astype(np.uint8)
        # ... and the reference scrub of the uploaded cells under the masks
        self.want_res = R.ref_batch(codec, k, m, img[:, :, :cell], self.masks)

    def slots(self):
        width = self.cell + PAD
        return [self.cells.data_ptr() + i * width for i in range(self.n)], [self.n * width] * self.n

    def uniform(self, cod, st=None):
        ptrs, strides = self.slots()
        cod.scrub_crc_device(ptrs, strides, self.cell, self.S, self.exp.data_ptr(), self.bad.data_ptr(),
                             self.res.data_ptr(), bytes_per_checksum=self.bpc, checksum_type=self.ctype,
                             stream=torch.cuda.current_stream().cuda_stream if st is None else st)

    def mixed(self, cod, ws=None, st=None):
        ptrs, strides = self.slots()
        if ws is None:
            ws = workspace(cod, self.S, self.cells.device)
        self.ws = ws
        cod.scrub_crc_device_mixed(ptrs, strides, self.masks, self.cell, self.S, self.exp.data_ptr(),
                                   self.bad.data_ptr(), self.res.data_ptr(), ws.data_ptr(), ws.numel(),
                                   bytes_per_checksum=self.bpc, checksum_type=self.ctype,
                                   stream=torch.cuda.current_stream().cuda_stream if st is None else st)

    def call(self, cod):
        self.mixed(cod) if self.mixed_form else self.uniform(cod)

    def check(self, what=""):
        torch.cuda.synchronize()
        got_res = as_u64(self.res, self.S)
        got_bad = self.bad.cpu().numpy()
        print(what, "results", got_res.tolist(), "flags", np.argwhere(got_bad).tolist())
        assert np.array_equal(got_res, self.want_res), (what, got_res.tolist(), self.want_res.tolist())
        assert np.array_equal(got_bad, self.want_bad), (what, np.argwhere(got_bad != self.want_bad).tolist())
        assert np.array_equal(self.cells.cpu().numpy(), self.h_cells), (what, "cells were written")
        assert np.array_equal(self.exp.cpu().numpy(), self.h_sums), (what, "expected sums were written")

    def check_against_existing_calls(self, cod, what=""):
        """The composition a caller runs today, on the same buffers:
        scrub_device[_mixed] for the results, checksum_verify_device over all
        k+m slots with the missing units' flags dropped for the flags."""
        dev_ = self.cells.device
        ptrs, strides = self.slots()
        res2 = prefilled(self.S, dev_)
        st = torch.cuda.current_stream().cuda_stream
        if self.mixed_form:
            ws2 = torch.empty(max(cod.scrub_mixed_workspace_size(self.S), 1), dtype=torch.uint8, device=dev_)
            cod.scrub_device_mixed(ptrs, strides, self.masks, self.cell, self.S, res2.data_ptr(), ws2.data_ptr(),
                                   ws2.numel(), st)
        else:
            cod.scrub_device(ptrs, strides, self.cell, self.S, res2.data_ptr(), st)
        bad2 = torch.zeros((self.S, self.n), dtype=torch.uint8, device=dev_)
        cod.checksum_verify_device(self.ctype, ptrs, strides, self.cell, self.S, self.bpc, self.exp.data_ptr(),
                                   bad2.data_ptr(), st)
        torch.cuda.synchronize()
        bad2 = bad2.cpu().numpy() * self.present
        preset = self.want_bad & ~((RC.chunk_sums(self.h_cells[:, :, :self.cell], self.bpc, self.ctype)
                                    != self.h_sums).any(axis=(2, 3)) & self.present).astype(np.uint8)
        assert np.array_equal(as_u64(self.res, self.S), as_u64(res2, self.S)), what
        assert np.array_equal(self.bad.cpu().numpy(), bad2 | preset), what


def workspace(cod, stripes, dev):
    """Exactly the advertised size, pre-filled."""
    return torch.full((max(cod.scrub_crc_mixed_workspace_size(stripes), 1),), SENT, dtype=torch.uint8, device=dev)


def clean(codec, k, m, S, cell, bpc=512, ctype=C32C):
    """Writable copies of the shared truth and of its sums."""
    return (np.array(RC.truth(k, m, S, cell, codec)), np.array(RC.true_sums(k, m, S, cell, codec, bpc, ctype)))


def resum(cells, sums, s, u, bpc=512, ctype=C32C):
    """The sums of cell (s, u) recomputed from its present bytes."""
    sums[s, u] = RC.chunk_sums(cells[s, u], bpc, ctype)


# ---- 1. clean -----------------------------------------------------------------------

FUSED_KE = [(k, e) for k in (2, 3, 6, 10) for e in (1, 2, 3, 4)]


@pytest.mark.parametrize("ctype", [C32C, C32], ids=["crc32c", "crc32"])
@pytest.mark.parametrize("k,e", FUSED_KE, ids=[f"k{k}-e{e}" for k, e in FUSED_KE])
def test_clean(dev, k, e, ctype):
    """Every (K, E) instantiation of the fused kernel, both kinds, every cell
    length: RS(k, e) with every unit present, and RS(k, 4) with 4 - e units
    missing (survivors and extras then include parity units)."""
    S = 3
    for cell in CELLS:
        cells, sums = clean("rs", k, e, S, cell, ctype=ctype)
        b = Batch("rs", k, e, cells, sums, dev, ctype=ctype)
        b.uniform(coder(k, e))
        b.check(("uniform", k, e, cell))
        assert not b.want_res.any() and not b.want_bad.any()
        if e < 4:
            n = k + 4
            cells, sums = clean("rs", k, 4, S, cell, ctype=ctype)
            masks = [lose(n, [(s + j) % n for j in range(4 - e)]) for s in range(S)]
            b = Batch("rs", k, 4, cells, sums, dev, masks=masks, ctype=ctype)
            b.mixed(coder(k, 4))
            b.check(("mixed", k, e, cell))
            assert not b.want_res.any() and not b.want_bad.any()


# ---- 2. equals the composition --------------------------------------------------------

def boundary_positions(cell):
    pos = {0, cell - 1}
    for step in (512, 1024, 4096, 8192, 32768):
        for b in range(step, cell, step):
            pos.update((b - 1, b))
    return sorted(p for p in pos if 0 <= p < cell)


def targets(k, n, mask, rot):
    """A survivor, an extra, a data unit and a parity unit of the mask, in turn
    (rotated by rot); where the mask has no extra the last survivor stands in."""
    pres = R.present_units(n, mask)
    surv, extra = pres[:k], pres[k:]
    data = [u for u in pres if u < k]
    par = [u for u in pres if u >= k]
    order = [surv[0], (extra or surv)[-1], data[-1] if data else pres[0], par[0] if par else pres[-1]]
    return order[rot % 4:] + order[:rot % 4]


def corrupt_batch(k, m, S, cell, masks, rot):
    """The corruption kinds of the issue, one per stripe (S >= 9)."""
    n = k + m
    cells, sums = clean("rs", k, m, S, cell)
    preset = []
    t = [targets(k, n, masks[s], rot + s) for s in range(S)]
    # 0: a byte flipped, the sums left alone
    cells[0, t[0][0], 700 % cell] ^= 0x40
    # 1: a byte flipped and its chunk sum recomputed to match (HDFS-15759)
    cells[1, t[1][0], 513 % cell] ^= 0x01
    resum(cells, sums, 1, t[1][0])
    # 2: only a sums word changed
    sums[2, t[2][0], (cell - 1) // 512, 3] ^= 0x80
    # 3: two units changed, one silently
    a, b = t[3][0], next(u for u in t[3][1:] + R.present_units(n, masks[3]) if u != t[3][0])
    cells[3, a, 0] ^= 0xFF
    cells[3, b, cell // 2] ^= 0x02
    resum(cells, sums, 3, b)
    # 4: flips at byte 0, at cell_len - 1 and on both sides of every boundary
    for p in boundary_positions(cell):
        cells[4, t[4][0], p] ^= 0x10
    # 5: the same positions, silently
    for p in boundary_positions(cell):
        cells[5, t[5][0], p] ^= 0x08
    resum(cells, sums, 5, t[5][0])
    # 6: a flip inside the short last chunk
    cells[6, t[6][0], cell - 3] ^= 0x20
    # 7: a pre-set flag on a clean unit must survive
    preset.append((7, t[7][0]))
    # 8 (and any further stripe): clean
    return cells, sums, preset


SHAPES = [(6, 3), (10, 4), (3, 2), (2, 1)]
EQ = [(k, m, S, form, rot) for (k, m) in SHAPES for S in (9, 17) for form in ("uniform", "degraded")
      for rot in range(4)]


@pytest.mark.parametrize("k,m,S,form,rot", EQ, ids=[f"rs-{k}-{m}-S{S}-{f}-r{r}" for k, m, S, f, r in EQ])
def test_equals_composition(dev, k, m, S, form, rot):
    """Batches of 9 and 17 stripes (the 8-stripe tile groups wrap).  uniform:
    every unit present, the uniform call.  degraded: stripe s lacks data unit
    s mod k, so a parity unit is among the survivors and e = m - 1 (RS(2,1):
    e == 0, sums only), the mixed call."""
    n, cell = k + m, 50192
    masks = [full(n)] * S if form == "uniform" else [lose(n, [s % k]) for s in range(S)]
    cells, sums, preset = corrupt_batch(k, m, S, cell, masks, rot)
    b = Batch("rs", k, m, cells, sums, dev, masks=None if form == "uniform" else masks, preset=preset)
    b.call(coder(k, m))
    b.check((k, m, S, form, rot))
    # what the cases are there to show, from the references alone
    e = m if form == "uniform" else m - 1
    t0 = targets(k, n, masks[0], rot)[0]
    assert b.want_bad[0, t0] == 1 and (e == 0 or b.want_res[0, 1] == 1)
    t1 = targets(k, n, masks[1], rot + 1)[0]
    assert b.want_bad[1, t1] == 0 and (e == 0 or b.want_res[1, 1] == 1)
    if e >= 2:
        for s, t in ((0, t0), (1, t1)):
            unit = ctypes.c_int(-1)
            v = H.lib.hec_scrub_verdict(int(b.want_res[s, 0]), int(b.want_res[s, 1]), n, ctypes.byref(unit))
            assert (v, unit.value) == (H.HEC_SCRUB_LOCATED, t)
    assert b.want_bad[2].sum() == 1 and tuple(b.want_res[2]) == (0, 0)
    assert b.want_bad[7].sum() == 1 and tuple(b.want_res[7]) == (0, 0)
    b.check_against_existing_calls(coder(k, m), (k, m, S, form, rot))


# ---- 3. mixed masks ---------------------------------------------------------------------

def node_failure_masks(n, S):
    """Stripe s lacks unit s mod (n + 1); index n = nothing lost.  No two
    neighbouring stripes share a mask."""
    return [full(n) if s % (n + 1) == n else lose(n, [s % (n + 1)]) for s in range(S)]


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)], ids=["rs-6-3", "rs-10-4"])
@pytest.mark.parametrize("cell", [528, 9232])
def test_after_one_node_failure(dev, k, m, cell):
    n, S = k + m, 24
    masks = node_failure_masks(n, S)
    assert all(a != b for a, b in zip(masks, masks[1:]))
    cells, sums = clean("rs", k, m, S, cell)
    for s in (1, 5, n, 17, 23):  # survivor, extra, the complete stripe, ...
        u = R.present_units(n, masks[s])[(3 * s) % (n - 1)]
        cells[s, u, (37 * s) % cell] ^= 0x04
        if s in (1, 17):  # silently
            resum(cells, sums, s, u)
    sums[2, R.present_units(n, masks[2])[0], 0, 0] ^= 1
    b = Batch("rs", k, m, cells, sums, dev, masks=masks)
    b.mixed(coder(k, m))
    b.check((k, m, cell))
    assert b.want_res[:, 1].astype(bool).sum() == 5 and b.want_bad.sum() == 4
    b.check_against_existing_calls(coder(k, m))


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4), (3, 2)], ids=["rs-6-3", "rs-10-4", "rs-3-2"])
def test_every_e_and_unchecked_stripes(dev, k, m):
    """e = m, ..., 1, 0 in one batch, then fewer than k units, then none; each
    kind twice (clean, and with a checksum-visible flip)."""
    n, cell = k + m, 9232
    losts = [list(range(1, 1 + j)) for j in range(m + 1)] + [list(range(m + 1)), list(range(1, n)), list(range(n))]
    masks = [lose(n, l) for l in losts for _ in range(2)]
    S = len(masks)
    assert S <= 24
    cells, sums = clean("rs", k, m, S, cell)
    for s in range(1, S, 2):
        pres = R.present_units(n, masks[s])
        if pres:
            cells[s, pres[-1], 9231 - s] ^= 0x80
    b = Batch("rs", k, m, cells, sums, dev, masks=masks)
    b.mixed(coder(k, m))
    b.check((k, m))
    # stripes with e == 0 or fewer than k units: (0, 0), their flips still flagged
    for s in range(2 * m, S):
        assert tuple(b.want_res[s]) == (0, 0)
    assert b.want_bad.sum() == (S - 2) // 2
    # the workspace past the call's image is the caller's: still the fill
    assert b.ws.numel() == coder(k, m).scrub_crc_mixed_workspace_size(S)
    b.check_against_existing_calls(coder(k, m))


def test_no_unit_anywhere(dev):
    """Every mask empty: results zeroed, nothing read, no workspace needed."""
    k, m, n, S, cell = 6, 3, 9, 5, 528
    cells, sums = clean("rs", k, m, S, cell)
    b = Batch("rs", k, m, cells, sums, dev, masks=[0] * S)
    ptrs, strides = b.slots()
    coder(k, m).scrub_crc_device_mixed(ptrs, strides, b.masks, cell, S, b.exp.data_ptr(), b.bad.data_ptr(),
                                       b.res.data_ptr(), None, 0, stream=torch.cuda.current_stream().cuda_stream)
    b.check()


# ---- 4. composed route, same results ------------------------------------------------------

COMPOSED = [("rs", 4, 2, 1008, 512, 0), ("xor", 5, 1, 1008, 512, 0), ("rs", 6, 6, 528, 512, 0),
            ("rs", 6, 3, 1000, 512, 0), ("rs", 6, 3, 37, 512, 0), ("rs", 4, 2, 1000, 512, 0),
            ("rs", 6, 3, 528, 256, 0), ("rs", 6, 3, 9232, 4096, 0), ("rs", 6, 3, 528, 512, 8)]


@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("codec,k,m,cell,bpc,base_off", COMPOSED,
                         ids=[f"{c}-{k}-{m}-{cell}-bpc{b}-off{o}" for c, k, m, cell, b, o in COMPOSED])
def test_composed_route(dev, codec, k, m, cell, bpc, base_off, form):
    """Other k, e = 6, cell lengths that are no multiple of 16, other chunk
    sizes, a base 8 bytes off the 16-B grid."""
    n, S = k + m, 9
    cells, sums = clean(codec, k, m, S, cell, bpc=bpc)
    masks = None
    if form == "mixed":
        masks = [full(n) if s % 3 == 0 else lose(n, [s % n]) for s in range(S)]
        if m > 1:
            masks[8] = lose(n, list(range(m)))  # e == 0
    pres = [R.present_units(n, full(n) if masks is None else masks[s]) for s in range(S)]
    cells[0, pres[0][0], cell - 1] ^= 0x40
    cells[4, pres[4][-1], 0] ^= 0x01
    resum(cells, sums, 4, pres[4][-1], bpc=bpc)
    sums[6, pres[6][1], 0, 1] ^= 0x02
    cells[8, pres[8][0], cell // 2] ^= 0x04
    b = Batch(codec, k, m, cells, sums, dev, masks=masks, base_off=base_off, bpc=bpc)
    if base_off:
        assert b.cells.data_ptr() % 16 == base_off
    b.call(coder(k, m, codec))
    b.check((codec, k, m, cell, bpc, base_off, form))
    assert b.want_bad.sum() == 3


# ---- 5. HEC_CHECKSUM_NULL -------------------------------------------------------------------

@pytest.mark.parametrize("form", ["uniform", "mixed"])
def test_checksum_null_is_the_plain_scrub(dev, form):
    k, m, n, S, cell = 6, 3, 9, 9, 9232
    cells, sums = clean("rs", k, m, S, cell)
    cells[2, 4, 100] ^= 0x01
    cells[7, 8, 9000] ^= 0x01
    masks = None if form == "uniform" else [lose(n, [s % 2]) for s in range(S)]
    b = Batch("rs", k, m, cells, sums, dev, masks=masks)
    ptrs, strides = b.slots()
    st = torch.cuda.current_stream().cuda_stream
    cod = coder(k, m)
    if form == "uniform":
        cod.scrub_crc_device(ptrs, strides, cell, S, None, None, b.res.data_ptr(), checksum_type=H.CHECKSUM_NULL,
                             stream=st)
    else:
        ws = workspace(cod, S, dev)
        cod.scrub_crc_device_mixed(ptrs, strides, b.masks, cell, S, None, None, b.res.data_ptr(), ws.data_ptr(),
                                   ws.numel(), checksum_type=H.CHECKSUM_NULL, stream=st)
    b.want_bad[:] = 0  # no checksum type: no flag, although two units do not match their sums
    b.check(form)
    assert b.want_res[:, 1].tolist().count(1) == 2


# ---- 6. graph capture --------------------------------------------------------------------------

def test_graph_capture_replay(dev):
    """The uniform call captured on one stream; replayed twice with a
    corruption added between the replays."""
    k, m, S, cell = 6, 3, 9, 50192
    cod = coder(k, m)
    cells, sums = clean("rs", k, m, S, cell)
    cells[3, 7, 40000] ^= 0x01
    b = Batch("rs", k, m, cells, sums, dev)
    b.uniform(cod)
    b.check("eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.uniform(cod, st=torch.cuda.current_stream().cuda_stream)
    b.res.fill_(-1)
    b.bad.zero_()
    torch.cuda.synchronize()
    g.replay()
    b.check("replay 0")
    # a second, silent corruption and a sums word: new references, same buffers
    cells[5, 1, 12345] ^= 0x80
    resum(cells, sums, 5, 1)
    sums[8, 0, 3, 0] ^= 0x01
    b2 = Batch("rs", k, m, cells, sums, dev)
    b.cells.copy_(b2.cells)
    b.exp.copy_(b2.exp)
    b.h_cells, b.h_sums, b.want_res, b.want_bad = b2.h_cells, b2.h_sums, b2.want_res, b2.want_bad
    b.res.fill_(-1)
    b.bad.zero_()
    torch.cuda.synchronize()
    g.replay()
    b.check("replay 1")
    assert b.want_res[:, 1].tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 0] and b.want_bad.sum() == 2


# ---- 7. two streams ----------------------------------------------------------------------------

def test_two_mixed_calls_on_two_streams(dev):
    k, m, n, S, cell = 6, 3, 9, 24, 50192
    cod = coder(k, m)
    batches = []
    for call in range(2):
        cells, sums = clean("rs", k, m, S, cell)
        masks = node_failure_masks(n, S)[call:] + node_failure_masks(n, S)[:call]
        u = R.present_units(n, masks[3 + call])[2]
        cells[3 + call, u, 77] ^= 0x01
        batches.append(Batch("rs", k, m, cells, sums, dev, masks=masks, seed=call))
    streams = [torch.cuda.Stream() for _ in range(2)]
    spaces = [workspace(cod, S, dev) for _ in range(2)]
    torch.cuda.synchronize()
    for b, st, ws in zip(batches, streams, spaces):
        with torch.cuda.stream(st):
            b.mixed(cod, ws=ws)
    for i, b in enumerate(batches):
        b.check(i)


# ---- 8. the loop from INTEGRATION.md -------------------------------------------------------------

def test_scrub_repair_scrub_loop(dev):
    """One silent corruption, one checksum-visible corruption and one lost unit
    in different stripes: scrub with sums -> new masks -> verified
    reconstruction in place on the same sums array -> final scrub with sums."""
    k, m, n, S, cell = 6, 3, 9, 9, 9232
    cod = coder(k, m)
    truth, tsums = clean("rs", k, m, S, cell)
    cells, sums = truth.copy(), tsums.copy()
    cells[1, 2, 5000] ^= 0x01  # silent: its sums were computed from the wrong bytes
    resum(cells, sums, 1, 2)
    cells[4, 7, 16] ^= 0x01    # checksum-visible
    masks = [full(n)] * S
    masks[6] = lose(n, [0])    # a lost unit
    b = Batch("rs", k, m, cells, sums, dev, masks=masks)
    b.mixed(cod)
    b.check("first scrub")
    res = as_u64(b.res, S)
    bad = b.bad.cpu().numpy()
    # flagged units leave the masks (their stripes would be scrubbed again
    # degraded; here m - 1 = 2 checks remain and nothing else is wrong), then
    # LOCATED units
    for s, u in np.argwhere(bad):
        masks[s] &= ~(1 << int(u))
    for s in range(S):
        unit = ctypes.c_int(-1)
        if H.lib.hec_scrub_verdict(int(res[s, 0]), int(res[s, 1]), n, ctypes.byref(unit)) == H.HEC_SCRUB_LOCATED:
            masks[s] &= ~(1 << unit.value)
    assert masks[1] == lose(n, [2]) and masks[4] == lose(n, [7]) and masks[6] == lose(n, [0])
    # the same images under the new masks (flagged and located units are now
    # missing slots: never read)
    b2 = Batch("rs", k, m, b.h_cells, b.h_sums, dev, masks=masks, raw=True)
    b2.mixed(cod)
    b2.check("degraded scrub")
    assert not b2.want_res.any() and not b2.want_bad.any()
    # repair in place, the rebuilt units' sums written into the same array
    rbad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
    ptrs, strides = b2.slots()
    ws = torch.empty(cod.reconstruct_crc_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    cod.reconstruct_crc_device_mixed(ptrs, strides, ptrs, strides, masks, None, cell, S, b2.exp.data_ptr(),
                                     ws.data_ptr(), ws.numel(), expected_ptr=b2.exp.data_ptr(),
                                     bad_ptr=rbad.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not rbad.any()
    # the end state: bytes, parity and sums all agree, and equal the truth
    final = Batch("rs", k, m, b2.cells.cpu().numpy(), b2.exp.cpu().numpy(), dev, raw=True)
    final.uniform(cod)
    final.check("final scrub")
    assert not final.want_res.any() and not final.want_bad.any()
    assert np.array_equal(final.h_cells[:, :, :cell], truth)
    assert (final.h_cells[:, :, cell:] == GARBAGE).all()
    assert np.array_equal(final.h_sums, tsums)


# ---- 9. arguments ----------------------------------------------------------------------------------

def test_invalid_arguments_queue_nothing(dev):
    """Every HEC_ERR_INVALID_ARG case of the header returns with nothing
    queued: all four buffers keep their fill."""
    k, m, n, S, cell = 6, 3, 9, 4, 528
    cod = coder(k, m)
    cells, sums = clean("rs", k, m, S, cell)
    cells[1, 1, 1] ^= 1  # a call that got through would flag and report it
    b = Batch("rs", k, m, cells, sums, dev, masks=[full(n)] * S)
    ws = workspace(cod, S, dev)
    ptrs, strides = b.slots()
    INV = H.HEC_ERR_INVALID_ARG
    masks = (ctypes.c_uint64 * S)(*b.masks)
    P = ctypes.c_void_p

    def call(mixed, handle=cod.handle, ctype=C32C, shards="ok", strd="ok", cell_len=cell, stripes=S, bpc=512,
             exp=b.exp.data_ptr(), bad=b.bad.data_ptr(), res=b.res.data_ptr(), present=masks, wsp=ws.data_ptr(),
             wsb=ws.numel()):
        sh = H._pp(ptrs) if shards == "ok" else shards
        sd = H._sp(strides) if strd == "ok" else strd
        if mixed:
            return H.lib.hec_scrub_crc_device_mixed(handle, ctype, sh, sd, present, cell_len, stripes, bpc, P(exp),
                                                    P(bad), P(res), P(wsp), wsb, None)
        return H.lib.hec_scrub_crc_device(handle, ctype, sh, sd, cell_len, stripes, bpc, P(exp), P(bad), P(res), None)

    holed = list(ptrs)
    holed[4] = 0
    for mixed in (False, True):
        assert call(mixed, handle=None) == INV
        assert call(mixed, shards=None) == INV
        assert call(mixed, strd=None) == INV
        assert call(mixed, res=None) == INV
        assert call(mixed, shards=H._pp(holed)) == INV
        assert call(mixed, cell_len=0) == INV
        assert call(mixed, bpc=0) == INV
        assert call(mixed, res=b.res.data_ptr() + 4) == INV
        assert call(mixed, exp=b.exp.data_ptr() + 2) == INV
        assert call(mixed, exp=None) == INV
        assert call(mixed, bad=None) == INV
        assert call(mixed, ctype=77) == INV
        assert call(mixed, stripes=0) == H.HEC_OK
    assert call(True, present=None) == INV
    assert call(True, wsp=None) == INV
    assert call(True, wsp=ws.data_ptr() + 8) == INV
    assert call(True, wsb=ws.numel() - 1) == INV
    torch.cuda.synchronize()
    assert (b.res == -1).all() and not b.bad.any()
    assert (ws == SENT).all()
    assert np.array_equal(b.cells.cpu().numpy(), b.h_cells) and np.array_equal(b.exp.cpu().numpy(), b.h_sums)


def test_batch_wrappers(dev):
    """scrub_crc_batch / scrub_crc_batch_mixed return (results, bad)."""
    k, m, n, S, cell = 6, 3, 9, 9, 528
    cod = coder(k, m)
    cells, sums = clean("rs", k, m, S, cell)
    cells[2, 3, 10] ^= 1
    masks = [lose(n, [s % 3]) for s in range(S)]
    for mk in (None, masks):
        b = Batch("rs", k, m, cells, sums, dev, masks=mk)
        packed = b.cells[:, :, :cell].contiguous()
        if mk is None:
            res, bad = H.scrub_crc_batch(cod, packed, b.exp)
        else:
            res, bad = H.scrub_crc_batch_mixed(cod, packed, mk, b.exp)
        torch.cuda.synchronize()
        assert np.array_equal(res.cpu().numpy().view(np.uint64), b.want_res)
        assert np.array_equal(bad.cpu().numpy(), b.want_bad)
