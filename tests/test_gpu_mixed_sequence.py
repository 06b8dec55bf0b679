"""The four per-stripe ("mixed") device calls share the coder's two pinned
staging images.  Here they follow one another on one coder and one stream with
no synchronise in between -- decode, reconstruct, scrub, verified reconstruct,
decode again -- so each image is refilled at least twice while earlier uploads
may still be queued.  Every output must equal, byte for byte, what the same
call gives when it runs alone and is followed by a synchronise; the decode and
the reconstruction are also held against the stripes that were encoded."""
import numpy as np
import pytest

import hdfs_native_ec as H
from test_gpu_reconstruct_crc import GARBAGE, coder, dev, present_mask, slots, stream, true_sums, truth  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S, CELL = 8, 1024  # one wave tile per cell: the smallest the register kernels take


class Calls:
    """Fresh buffers for the five calls of the sequence, each call with its
    own inputs, outputs and workspace (None where the variant passes none)."""

    def __init__(self, k, m, losts, dev, null_workspaces):
        self.cod, self.k, self.n = coder(k, m), k, k + m
        cod, n = self.cod, self.n
        t = truth(k, m, S, CELL)
        self.masks = [present_mask(n, lost) for lost in losts]

        def degraded(corrupt=None, lost_units=losts):
            cells = torch.from_numpy(t.copy()).to(dev)
            if corrupt is not None:
                cells[corrupt] ^= 0x40
            for s, lost in enumerate(lost_units):
                for i in lost:
                    cells[s, i] = GARBAGE
            return cells

        def workspace(size, absent=False):
            return None if absent else torch.empty(size, dtype=torch.uint8, device=dev)

        # the second decode takes the patterns in reverse order: another image in the same pinned buffer
        self.dec = [(degraded(lost_units=order), torch.full((S, k, CELL), 0xA5, dtype=torch.uint8, device=dev),
                     workspace(cod.decode_mixed_workspace_size(S), null_workspaces),
                     [present_mask(n, lost) for lost in order])
                    for order in (losts, losts[::-1])]
        self.rec = (degraded(), workspace(cod.reconstruct_mixed_workspace_size(S), null_workspaces))
        # a corrupt byte in the one stripe that has every unit (stripe 0)
        self.scr = (degraded(corrupt=(0, 1, 77)), torch.full((S, 2), -1, dtype=torch.int64, device=dev),
                    workspace(cod.scrub_mixed_workspace_size(S)))
        sums = torch.from_numpy(true_sums(k, m, S, CELL).copy()).to(dev)  # [S, n, 2, 4]
        self.crc = (degraded(), torch.full(tuple(sums.shape), 0xA5, dtype=torch.uint8, device=dev), sums,
                    torch.zeros((S, n), dtype=torch.uint8, device=dev),
                    workspace(cod.reconstruct_crc_mixed_workspace_size(S)))

    @staticmethod
    def _ws(w):
        return (0, 0) if w is None else (w.data_ptr(), w.numel())

    def decode(self, which):
        cells, out, ws, masks = self.dec[which]
        ptrs, strides = slots(cells)
        optrs, ostrides = slots(out)
        self.cod.decode_device_mixed(ptrs, strides, optrs, ostrides, masks, CELL, S, *self._ws(ws), stream=stream())

    def reconstruct(self):
        cells, ws = self.rec
        ptrs, strides = slots(cells)
        self.cod.reconstruct_device_mixed(ptrs, strides, ptrs, strides, self.masks, None, CELL, S, *self._ws(ws),
                                          stream=stream())

    def scrub(self):
        cells, results, ws = self.scr
        ptrs, strides = slots(cells)
        self.cod.scrub_device_mixed(ptrs, strides, self.masks, CELL, S, results.data_ptr(), *self._ws(ws),
                                    stream=stream())

    def reconstruct_crc(self):
        cells, sums, expected, bad, ws = self.crc
        ptrs, strides = slots(cells)
        self.cod.reconstruct_crc_device_mixed(ptrs, strides, ptrs, strides, self.masks, None, CELL, S, sums.data_ptr(),
                                              *self._ws(ws), expected_ptr=expected.data_ptr(), bad_ptr=bad.data_ptr(),
                                              bytes_per_checksum=512, checksum_type=H.CHECKSUM_CRC32C, stream=stream())

    def sequence(self):
        return [("decode", lambda: self.decode(0), lambda: [self.dec[0][1]]),
                ("reconstruct", self.reconstruct, lambda: [self.rec[0]]),
                ("scrub", self.scrub, lambda: [self.scr[1]]),
                ("reconstruct_crc", self.reconstruct_crc, lambda: [self.crc[0], self.crc[1], self.crc[3]]),
                ("decode again", lambda: self.decode(1), lambda: [self.dec[1][1]])]


@pytest.mark.parametrize("k,m,losts,null_workspaces", [
    # the register kernels' shape: zero, one and three units missing, runs and repeats
    (6, 3, [(), (1,), (0, 4, 7), (0, 4, 7), (), (6,), (2, 3, 5), (1,)], False),
    # k = 4 is outside the register kernels' set: per run of stripes or by bytes, no decode / reconstruct workspace
    (4, 2, [(), (1,), (0, 4), (0, 4), (), (5,), (2, 3), (1,)], True),
], ids=["rs63", "rs42-null-workspaces"])
def test_mixed_calls_back_to_back_share_the_pinned_images(dev, k, m, losts, null_workspaces):
    t = truth(k, m, S, CELL)
    alone = {}
    ref = Calls(k, m, losts, dev, null_workspaces)
    for name, launch, outputs in ref.sequence():
        launch()
        torch.cuda.synchronize()
        alone[name] = [o.clone() for o in outputs()]
    # the reference itself: rebuilt data where it was missing, untouched elsewhere; every unit repaired
    for name, order in (("decode", losts), ("decode again", losts[::-1])):
        want = np.full((S, k, CELL), 0xA5, dtype=np.uint8)
        for s, lost in enumerate(order):
            for i in (i for i in lost if i < k):
                want[s, i] = t[s, i]
        assert np.array_equal(alone[name][0].cpu().numpy(), want), name
    assert np.array_equal(alone["reconstruct"][0].cpu().numpy(), t)
    assert np.array_equal(alone["reconstruct_crc"][0].cpu().numpy(), t)
    assert alone["scrub"][0][0, 1].item() != 0 and not alone["scrub"][0][1:, 1].any()  # bad bytes in stripe 0 only

    seq = Calls(k, m, losts, dev, null_workspaces)
    steps = seq.sequence()
    for _, launch, _ in steps:
        launch()
    torch.cuda.synchronize()
    for name, _, outputs in steps:
        for i, (got, exp) in enumerate(zip(outputs(), alone[name])):
            assert torch.equal(got, exp), (name, i)
