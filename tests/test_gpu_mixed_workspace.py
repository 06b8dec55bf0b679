"""The workspace of the five per-stripe ("mixed") device calls, as the device
got it.  Each call runs on the worst batch its *_workspace_size promises to
cover -- every distinct pattern once -- and on half of it (the stripe-count
cap of the size functions), with a workspace of exactly the advertised size:
a 256-byte aligned slice of a larger tensor with 4 KiB of 0x5C on either side.
After one synchronize both bands must be intact and the results exact against
the references the other files use (the stripes that were encoded, the
oracle's chunk sums, degraded_scrub_ref).  For the three plain calls at the
register kernels' shapes the per-stripe plan offsets and the plan headers they
point at are read back and held against a presence mask's own definition of
survivors and targets.  A last test walks the free-and-regrow path of the
coder's two pinned staging images with uploads still queued.

  shape     reaches
  --------  ---------------------------------------------------------------
  RS(3,2)   the register kernels (k = 3), 15 loss masks / 6 scrub masks
  RS(6,3)   the register kernels (k = 6), 129 loss masks / 46 scrub masks
  RS(5,3)   the byte kernel (scrub) and the per-run route (decode,
            reconstruction), 92 loss masks / 37 scrub masks
"""
import itertools

import numpy as np
import pytest

import degraded_scrub_ref as R
import hdfs_native_ec as H
import test_gpu_reconstruct_crc as RC
import test_gpu_scrub_crc as SC
from test_gpu_reconstruct_crc import dev  # noqa: F401  (fixture)
from test_gpu_scrub import as_u64, prefilled
from test_gpu_scrub_mixed import KINDS, corrupt, with_garbage

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD, BAND = 4096, 0x5C
CALLS = ("decode", "reconstruct", "scrub", "reconstruct_crc", "scrub_crc")
PLAIN = CALLS[:3]
SHAPES = [(3, 2), (6, 3), (5, 3)]
CELLS = (16, 528)
NO_PLAN = 0xFFFFFFFF


class Guarded:
    """Exactly `size` bytes on a 256-byte boundary (filled 0xA5) inside a larger
    tensor, with at least GUARD bytes of BAND before and after."""

    def __init__(self, size, dev):
        self.raw = torch.full((size + 2 * GUARD + 256,), BAND, dtype=torch.uint8, device=dev)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.size = size
        self.ws = self.raw[self.off:self.off + size]
        self.ws.fill_(0xA5)
        assert self.ws.data_ptr() % 256 == 0 and self.ws.numel() == size
        assert self.off >= GUARD and self.raw.numel() - self.off - size >= GUARD

    def assert_bands_intact(self, what):
        before, after = self.raw[:self.off], self.raw[self.off + self.size:]
        assert bool((before == BAND).all()), (what, "bytes before the workspace were written",
                                              (before != BAND).nonzero()[:8].flatten().tolist())
        assert bool((after == BAND).all()), (what, "bytes after the workspace were written",
                                             (after != BAND).nonzero()[:8].flatten().tolist())


def all_masks(call, k, m):
    """Every distinct pattern of the call once, in a fixed shuffled order: 1 ..
    m units lost (decode, reconstruction), fewer than m lost (scrub)."""
    n = k + m
    counts = range(0, m) if call.startswith("scrub") else range(1, m + 1)
    masks = [RC.present_mask(n, lost) for r in counts for lost in itertools.combinations(range(n), r)]
    rng = np.random.default_rng(100 * k + m + len(call))
    return [masks[i] for i in rng.permutation(len(masks))]


def lost_units(n, mask):
    return tuple(i for i in range(n) if not (mask >> i) & 1)


def ref_header(call, k, n, mask):
    """(survivors, targets, missing mask) of a stripe's plan by definition, or
    None where the stripe has nothing to compute."""
    pres, lost = R.present_units(n, mask), list(lost_units(n, mask))
    if call == "decode":
        targets, missing = [i for i in lost if i < k], 0
    elif call == "reconstruct":
        targets, missing = lost, 0
    else:
        targets, missing = pres[k:], sum(1 << i for i in lost)
    if not targets or len(pres) < k:
        return None
    return pres[:k], targets, missing


class Run:
    """One call: its buffers, its guarded workspace of exactly the advertised
    size, and what it must leave behind."""

    def __init__(self, call, cod, k, m, cell, masks, dev, seed=0):
        self.call, self.cod, self.k, self.m, self.n, self.cell = call, cod, k, m, k + m, cell
        self.masks, self.S = masks, len(masks)
        n, S = self.n, self.S
        self.what = f"{call} RS({k},{m}) cell={cell} S={S}"
        size = {"decode": cod.decode_mixed_workspace_size, "reconstruct": cod.reconstruct_mixed_workspace_size,
                "scrub": cod.scrub_mixed_workspace_size, "reconstruct_crc": cod.reconstruct_crc_mixed_workspace_size,
                "scrub_crc": cod.scrub_crc_mixed_workspace_size}[call](S)
        self.guard = Guarded(size, dev)
        t = RC.truth(k, m, S, cell)
        rng = np.random.default_rng(seed + 17 * S + cell)
        losts = [lost_units(n, mask) for mask in masks]
        if call in ("decode", "reconstruct"):
            self.cells = torch.from_numpy(t.copy()).to(dev)
            for s, lost in enumerate(losts):
                for i in lost:
                    self.cells[s, i] = RC.GARBAGE
            self.out = torch.full((S, k, cell), 0xA5, dtype=torch.uint8, device=dev)
            self.want_out = np.full((S, k, cell), 0xA5, dtype=np.uint8)
            for s, lost in enumerate(losts):
                for i in (i for i in lost if i < k):
                    self.want_out[s, i] = t[s, i]
        elif call == "scrub":
            cells = t.copy()
            for st in range(0, S, 2):
                corrupt(cells, st, k, masks[st], KINDS[(st // 2) % len(KINDS)], rng)
            self.want_res = R.ref_batch("rs", k, m, cells, masks)
            assert self.want_res[:, 1].any()
            self.cells = torch.from_numpy(with_garbage(cells, masks)).to(dev)
            self.res = prefilled(S, dev)
        elif call == "reconstruct_crc":
            # one corrupt byte in a survivor of stripe 1 (or 0): flagged, its targets unspecified
            s = min(1, S - 1)
            survivor = R.present_units(n, masks[s])[0]
            self.case = RC.mixed_case(cod, k, m, S, cell, losts, dev, corrupt=[(s, survivor, cell - 1)])
        else:
            cells, sums = SC.clean("rs", k, m, S, cell)
            for st in range(0, S, 3):  # a corrupt byte whose sum still matches the original: the parity check finds it
                pres = R.present_units(n, masks[st])
                cells[st, pres[int(rng.integers(0, len(pres)))], int(rng.integers(0, cell))] ^= 0x21
            for st in range(1, S, 5):  # a wrong expected sum over clean bytes: only the flag
                pres = R.present_units(n, masks[st])
                sums[st, pres[int(rng.integers(0, len(pres)))], -1, 0] ^= 0x80
            self.batch = SC.Batch("rs", k, m, cells, sums, dev, masks=masks)
            assert self.batch.want_res[:, 1].any() and self.batch.want_bad.any()

    def launch(self):
        cod, ws, S, cell = self.cod, self.guard.ws, self.S, self.cell
        if self.call == "decode":
            ptrs, strides = RC.slots(self.cells)
            optrs, ostrides = RC.slots(self.out)
            cod.decode_device_mixed(ptrs, strides, optrs, ostrides, self.masks, cell, S, ws.data_ptr(), ws.numel(),
                                    stream=RC.stream())
        elif self.call == "reconstruct":
            ptrs, strides = RC.slots(self.cells)
            cod.reconstruct_device_mixed(ptrs, strides, ptrs, strides, self.masks, None, cell, S, ws.data_ptr(),
                                         ws.numel(), stream=RC.stream())
        elif self.call == "scrub":
            ptrs, strides = RC.slots(self.cells)
            cod.scrub_device_mixed(ptrs, strides, self.masks, cell, S, self.res.data_ptr(), ws.data_ptr(), ws.numel(),
                                   RC.stream())
        elif self.call == "reconstruct_crc":
            self.case.mixed(workspace=ws)
        else:
            self.batch.mixed(cod, ws=ws)

    def check(self):
        """After a synchronize."""
        self.guard.assert_bands_intact(self.what)
        t = RC.truth(self.k, self.m, self.S, self.cell)
        if self.call == "decode":
            assert np.array_equal(self.out.cpu().numpy(), self.want_out), self.what
        elif self.call == "reconstruct":
            assert np.array_equal(self.cells.cpu().numpy(), t), self.what
        elif self.call == "scrub":
            got = as_u64(self.res, self.S)
            assert np.array_equal(got, self.want_res), (self.what, np.nonzero((got != self.want_res).any(axis=1))[0].tolist())
        elif self.call == "reconstruct_crc":
            self.case.check(self.what)
        else:
            self.batch.check(self.what)

    def check_readback(self):
        """[0, 4 * S) of the workspace and the headers the offsets point at."""
        k, n, S = self.k, self.n, self.S
        ws = self.guard.ws.cpu().numpy()
        offsets = ws[:4 * S].view("<u4")
        blob_pos = -(-4 * S // 256) * 256
        refs = [ref_header(self.call, k, n, mask) for mask in self.masks]
        if not any(refs):  # nothing to compute: the call returns before it touches the workspace
            assert (ws == 0xA5).all(), self.what
            return 0
        planned = 0
        for s, (mask, ref) in enumerate(zip(self.masks, refs)):
            o = int(offsets[s])
            if ref is None:
                assert o == NO_PLAN, (self.what, s, hex(mask), o)
                continue
            planned += 1
            surv, targets, missing = ref
            assert o != NO_PLAN and o % 16 == 0 and blob_pos + o + 64 <= ws.size, (self.what, s, hex(mask), o)
            h = ws[blob_pos + o:blob_pos + o + 64]
            assert int(h[:4].view("<u4")[0]) == len(targets), (self.what, s, hex(mask))
            assert h[4:36].tolist() == surv + [0] * (32 - k), (self.what, s, hex(mask), h[4:36].tolist())
            assert h[36:52].tolist() == targets + [0] * (16 - len(targets)), (self.what, s, hex(mask), h[36:52].tolist())
            assert int(h[52:60].view("<u8")[0]) == missing and not h[60:].any(), (self.what, s, hex(mask))
        return planned


CASES = [(call, k, m, cell, half) for call in CALLS for (k, m) in SHAPES for cell in CELLS for half in (False, True)]


@pytest.mark.parametrize("call,k,m,cell,half", CASES,
                         ids=[f"{c}-rs{k}{m}-{cell}-{'half' if h else 'all'}" for c, k, m, cell, h in CASES])
def test_guard_bands_and_results(dev, call, k, m, cell, half):
    masks = all_masks(call, k, m)
    assert len(masks) == {(3, 2): (15, 6), (6, 3): (129, 46), (5, 3): (92, 37)}[(k, m)][call.startswith("scrub")]
    if half:
        masks = masks[:len(masks) // 2]
    run = Run(call, RC.coder(k, m), k, m, cell, masks, dev)
    torch.cuda.synchronize()
    run.launch()
    torch.cuda.synchronize()
    run.check()
    if call in PLAIN and k in (3, 6):
        assert run.check_readback() == sum(ref_header(call, k, k + m, mask) is not None for mask in masks) > 0


@pytest.mark.parametrize("call", PLAIN)
def test_pinned_image_regrows_between_queued_uploads(dev, call):
    """A coder of its own, one stream, nothing synchronized in between: two
    small batches (each of the two pinned images is allocated small), every
    pattern (the first image is freed and regrown while the second one's
    upload may still be queued), a small batch again.  Every call has its own
    buffers and its own guarded workspace."""
    k, m, cell = 6, 3, 528
    every = all_masks(call, k, m)
    planned = [mask for mask in every if ref_header(call, k, k + m, mask) is not None]  # the small ones upload an image too
    cod = H.Coder(k, m, 0)
    try:
        runs = [Run(call, cod, k, m, cell, masks, dev, seed=i)
                for i, masks in enumerate((planned[:3], planned[3:6], every, planned[-3:]))]
        torch.cuda.synchronize()
        for run in runs:
            run.launch()
        torch.cuda.synchronize()
        for run in runs:
            run.check()
            assert run.check_readback() > 0
    finally:
        torch.cuda.synchronize()
        cod.close()
