"""Checksum-only reconstruction on the GPU: hec_reconstruct_sums_device (one
pattern per group, optional short last stripe) and
hec_reconstruct_sums_device_mixed (one pattern per stripe) -- the fused kernel
without its output stores and the byte-wise generic kernel.  Ground truth is
the CPU oracle throughout: the stripe that was encoded (random data plus the
oracle's parity rows) and the C oracle's chunk sums and CRCs of it.  The
whole-buffer-image discipline of test_gpu_reconstruct_crc.py: 0xEE between
cell_len and the stride and in lost slots, 0xA5 in every sums byte, zeroed
flags; after a call the ENTIRE cell buffer, sums buffer and flag buffer must
equal their expected images, so a write to any cell, to a sums word of a unit
that is no target or past a target's live chunks shows as well as a wrong sum."""
import ctypes

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H
from composite_crc_cases import data_len_cases, oracle_crc
from composite_crc_ref import cell_lengths
from test_gpu_reconstruct_crc import (CELLS, GARBAGE, SENT, chunk_sums, coder, patterns, present_mask, slots, stream,
                                      true_sums, truth)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32
GUARD = 0xC3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


class Case:
    """One call's buffers and their expected images.

    t [S, n, cell] are the true cells and true [S, n, nck, 4] their true sums
    with SENT in the slots no live chunk covers (lens[s][u] = the bytes of cell
    (s, u) that count; None = cell everywhere).  losts[s] = the units stripe s
    lacks, wants[s] = those whose sums are asked for (None: all of them).
    corrupt = [(stripe, unit, byte)]: that byte of a present cell is flipped;
    corrupt_sums = [(stripe, unit, chunk)]: that expected sum instead.
    expected: "sep" = a buffer of its own holding every true sum, "same" = the
    sums buffer itself (true sums at the present units' slots), None = no
    verification.  base_off moves the cell buffer's base off the 16-B grid."""

    def __init__(self, cod, t, true, losts, dev, wants=None, expected="sep", corrupt=(), corrupt_sums=(), pad=0,
                 base_off=0, bpc=512, ctype=C32C, lens=None, data_len=0):
        S, n, cell = t.shape
        self.cod, self.S, self.n, self.cell, self.bpc, self.ctype = cod, S, n, cell, bpc, ctype
        self.k, self.data_len = cod.data_units, data_len
        self.losts = [tuple(l) for l in losts]
        self.wants = [tuple(l) for l in losts] if wants is None else [tuple(w) for w in wants]
        self.have_want = wants is not None
        width = cell + pad
        self.raw = torch.full((S * n * width + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = self.raw[base_off:].view(S, n, width)
        self.cells[:, :, :cell] = torch.from_numpy(t.copy()).to(dev)
        if lens is not None:  # a short last stripe: nothing at or past n0 is the caller's
            n0 = max(lens[S - 1])
            self.cells[S - 1, :, n0:] = GARBAGE
        for (s, u, b) in corrupt:
            assert u not in self.losts[s]
            self.cells[s, u, b] ^= 0x40
        for s, lost in enumerate(self.losts):
            for i in lost:
                self.cells[s, i] = GARBAGE
        self.exp_raw = self.raw.clone()  # the call only reads the cells
        self.ts = torch.from_numpy(true.copy()).to(dev)  # [S, n, nck, 4]
        self.sums = torch.full(tuple(self.ts.shape), SENT, dtype=torch.uint8, device=dev)
        self.expected = None
        if expected == "sep":
            self.expected = self.ts.clone()
        elif expected == "same":
            for s, lost in enumerate(self.losts):
                keep = [i for i in range(n) if i not in lost]
                self.sums[s, keep] = self.ts[s, keep]
            self.expected = self.sums
        if expected is not None:
            for (s, u, c) in corrupt_sums:
                assert u not in self.losts[s]
                self.expected[s, u, c, 3] ^= 1
        self.exp_sums = self.sums.clone()
        for s, w in enumerate(self.wants):
            for i in w:
                self.exp_sums[s, i] = self.ts[s, i]  # SENT past the live chunks
        self.bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        self.exp_bad = torch.zeros((S, n), dtype=torch.uint8, device=dev)
        # a stripe's plan reads its first k present units, and only when the
        # stripe has a target
        self.dirty = set()
        for (s, u, _) in list(corrupt) + (list(corrupt_sums) if expected is not None else []):
            surv = [i for i in range(n) if i not in self.losts[s]][:self.k]
            if u in surv and self.wants[s]:
                self.dirty.add(s)
                if expected is not None:
                    self.exp_bad[s, u] = 1

    def chk_args(self):
        return dict(expected_ptr=None if self.expected is None else self.expected.data_ptr(),
                    bad_ptr=None if self.expected is None else self.bad.data_ptr(),
                    bytes_per_checksum=self.bpc, checksum_type=self.ctype)

    def uniform(self, strm=None):
        """One hec_reconstruct_sums_device call: every stripe lacks losts[0]."""
        assert len(set(self.losts)) == 1 and len(set(self.wants)) == 1
        ptrs, strides = slots(self.cells)
        shards = [None if i in self.losts[0] else ptrs[i] for i in range(self.n)]
        self.cod.reconstruct_sums_device(shards, strides, self.cell, self.S, self.sums.data_ptr(),
                                         want=list(self.wants[0]) if self.have_want else None,
                                         data_len=self.data_len, stream=stream() if strm is None else strm,
                                         **self.chk_args())

    def mixed(self, workspace=None, strm=None, null_units=()):
        """One hec_reconstruct_sums_device_mixed call."""
        ptrs, strides = slots(self.cells)
        ptrs = [None if i in null_units else p for i, p in enumerate(ptrs)]
        masks = [present_mask(self.n, l) for l in self.losts]
        wants = [sum(1 << i for i in w) for w in self.wants] if self.have_want else None
        if workspace is None:
            workspace = torch.empty(self.cod.reconstruct_crc_mixed_workspace_size(self.S), dtype=torch.uint8,
                                    device=self.cells.device)
        self.workspace = workspace
        self.cod.reconstruct_sums_device_mixed(ptrs, strides, masks, wants, self.cell, self.S, self.sums.data_ptr(),
                                               workspace.data_ptr(), workspace.numel(),
                                               stream=stream() if strm is None else strm, **self.chk_args())

    def check(self, what=""):
        """After a synchronize: everything equals its expected image; in a
        stripe that read a corrupt survivor the targets' sums are unspecified,
        everything else still holds."""
        assert torch.equal(self.bad, self.exp_bad), (what, "flags", self.bad.nonzero().tolist(),
                                                     self.exp_bad.nonzero().tolist())
        assert torch.equal(self.raw, self.exp_raw), (what, "a cell byte was written")
        got, exp = self.sums, self.exp_sums
        if self.dirty:
            got, exp = got.clone(), exp.clone()
            for s in self.dirty:
                for i in self.wants[s]:
                    got[s, i] = 0
                    exp[s, i] = 0
        if not torch.equal(got, exp):
            diff = (got != exp).reshape(self.S, self.n, -1).any(dim=2).nonzero().tolist()
            raise AssertionError((what, "sums", "stripe/unit pairs that differ", diff[:20]))

    def no_change(self, what=""):
        """Nothing was written: every buffer still holds its initial image."""
        assert not bool(self.bad.any()), what
        assert torch.equal(self.raw, self.exp_raw), what
        assert bool((self.sums == SENT).all()) or self.expected is self.sums, what


def uniform_case(cod, k, m, S, cell, lost, dev, want=None, codec="rs", **kw):
    bpc, ctype = kw.get("bpc", 512), kw.get("ctype", C32C)
    return Case(cod, truth(k, m, S, cell, codec), true_sums(k, m, S, cell, codec, bpc, ctype), [lost] * S, dev,
                wants=None if want is None else [want] * S, **kw)


def mixed_case(cod, k, m, S, cell, losts, dev, wants=None, codec="rs", **kw):
    bpc, ctype = kw.get("bpc", 512), kw.get("ctype", C32C)
    return Case(cod, truth(k, m, S, cell, codec), true_sums(k, m, S, cell, codec, bpc, ctype), losts, dev,
                wants=wants, **kw)


# ---- 1. fused shapes against the oracle -------------------------------------------

def lost_sets(k, m):
    """(lost, want): one data unit, one parity unit, the largest mixed set of
    at most 4 targets, and a want narrower than the loss."""
    t = min(m, 4)
    big = tuple(range(k - (t + 1) // 2, k + t // 2)) if t > 1 else (k - 1,)
    sets = [((1,), None), ((k + m - 1,), None), (big, None)]
    if t > 1:
        sets.append((big, (big[-1],)))
        sets.append(((0, k), (0,)))
    return sets


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (10, 4), (2, 2)])
def test_fused_shapes_against_oracle(dev, k, m, cell):
    """gf_reconstruct_crc without its stores: CRC32C with d_expected absent,
    separate and equal to d_sums; CRC32 where the cell is 528 or 9232."""
    S = 9 if cell < 50000 else 3
    cases = []
    for lost, want in lost_sets(k, m):
        for expected in (None, "sep", "same"):
            cases.append(uniform_case(coder(k, m), k, m, S, cell, lost, dev, want=want, expected=expected, pad=48))
        if cell in (528, 9232):
            cases.append(uniform_case(coder(k, m), k, m, S, cell, lost, dev, want=want, expected="same", ctype=C32))
    for c in cases:
        c.uniform()
    torch.cuda.synchronize()
    for c in cases:
        assert not c.dirty
        c.check((c.losts[0], c.wants[0], c.ctype, c.expected is not None))


# ---- 2. flags ---------------------------------------------------------------------

@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (10, 4, 528)])
def test_flags_exactly_the_corrupt_survivors(dev, k, m, cell, form):
    """A flipped byte in a survivor flags exactly that (stripe, unit): the
    first chunk, a middle chunk, the short last chunk, the last byte of a full
    chunk; a present unit the plan does not read is never flagged.  Then the
    same cells through a corrupt expected sum instead of corrupt data."""
    n, S = k + m, 9
    lost = (1,)  # survivors: 0, 2 .. k; units k+1 .. are present and unread
    nck = -(-cell // 512)
    spots = [(0, 0, 0), (2, 2, min((nck // 2) * 512 + 100, cell - 3)), (3, k, cell - 1), (5, 3, 511), (7, n - 1, 40),
             (8, 0, cell - 17), (8, 4, 512 + 5)]
    for by_sum in (False, True):
        kw = dict(corrupt_sums=[(s, u, b // 512) for (s, u, b) in spots]) if by_sum else dict(corrupt=spots)
        c = uniform_case(coder(k, m), k, m, S, cell, lost, dev, **kw)
        assert c.dirty == {0, 2, 3, 5, 8} and int(c.exp_bad.sum()) == 6
        c.uniform() if form == "uniform" else c.mixed()
        torch.cuda.synchronize()
        c.check((form, by_sum))


# ---- 3. the generic route, same images ----------------------------------------------

@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("shape", ["cell1000", "cell37", "bpc256", "bpc4096", "rs42", "xor51", "rs-legacy", "rs66", "base8"])
def test_generic_route_same_images(dev, shape, form):
    """The shapes the fused kernel does not take run gf_reconstruct_sums_bytes
    behind a verify pass over the survivors: same sums and flags."""
    k, m, codec, cell, kw = 6, 3, "rs", 9232, {}
    lost = (1, 7)
    if shape == "cell1000":
        cell = 1000
    elif shape == "cell37":
        cell = 37
    elif shape == "bpc256":
        kw["bpc"] = 256
    elif shape == "bpc4096":
        kw["bpc"] = 4096
    elif shape == "rs42":
        k, m, lost, cell = 4, 2, (0, 5), 1000
    elif shape == "xor51":
        k, m, codec, lost, cell = 5, 1, "xor", (3,), 1000
    elif shape == "rs-legacy":
        codec, cell = "rs-legacy", 1000
    elif shape == "rs66":
        k, m, lost, cell = 6, 6, (0, 2, 7, 9, 11), 1000  # 5 target rows: two launches
    elif shape == "base8":
        kw["base_off"] = 8
    n, S = k + m, 9
    cod = coder(k, m, codec)
    surv = [i for i in range(n) if i not in lost][:k]
    corrupt = [(3, surv[0], cell // 2), (5, surv[-1], cell - 1)]
    if form == "uniform":
        a = uniform_case(cod, k, m, S, cell, lost, dev, codec=codec, **kw)
        b = uniform_case(cod, k, m, S, cell, lost, dev, codec=codec, corrupt=corrupt, expected="same", **kw)
        c = uniform_case(cod, k, m, S, cell, lost, dev, codec=codec, expected=None, ctype=C32, **kw)
        cases = [a, b, c]
        for x in cases:
            x.uniform()
    else:
        pats = [()] + [p for p in patterns(n, 1, min(m, 2))] + [lost]
        losts = [pats[(5 * s + 1) % len(pats)] for s in range(S - 1)] + [lost]
        a = mixed_case(cod, k, m, S, cell, losts, dev, codec=codec, **kw)
        b = mixed_case(cod, k, m, S, cell, [lost] * S, dev, codec=codec, corrupt=corrupt, expected="same", **kw)
        cases = [a, b]
        for x in cases:
            x.mixed()
    if shape == "base8":
        assert a.cells.data_ptr() % 16 == 8
    torch.cuda.synchronize()
    assert b.dirty == {3, 5}
    for i, x in enumerate(cases):
        x.check((shape, form, i))


# ---- 4. short last stripe, followed by the composite --------------------------------

_clib = None


def clib():
    global _clib
    if _clib is None:
        _clib = O.load_c_oracle()
    return _clib


_groups = {}


def short_group(k, m, cell, S, data_len, ctype, bpc=512, seed=0):
    """A block group whose file has data_len bytes (0: every stripe full), once
    per shape, read-only: cells [S, n, cell] (random up to data_len, zeros
    behind it, the oracle's parity of that), lens [S][n], the true-length chunk
    sums [S, n, nck, 4] with SENT where no live chunk is, and the oracle's CRC
    of every unit's actual bytes and of the file."""
    key = (k, m, cell, S, data_len, ctype, bpc, seed)
    if key not in _groups:
        n = k + m
        rng = np.random.default_rng(1000 * k + cell + 7 * data_len + seed)
        logical = data_len or S * k * cell
        t = np.zeros((S, n, cell), dtype=np.uint8)
        data = rng.integers(0, 256, size=S * k * cell, dtype=np.uint8)
        data[logical:] = 0
        t[:, :k] = data.reshape(S, k, cell)
        par = O.matmul_shards(O.codec_matrix("rs", k, m)[k:], [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)])
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        lens = cell_lengths(n, k, cell, S, data_len)
        nck = -(-cell // bpc)
        sums = np.full((S, n, nck, 4), SENT, dtype=np.uint8)
        for s in range(S):
            for u in range(n):
                if lens[s][u]:
                    live = chunk_sums(t[s, u, :lens[s][u]], bpc, ctype)
                    sums[s, u, :live.shape[0]] = live
        units = [oracle_crc(clib(), ctype, np.concatenate([t[s, u, :lens[s][u]] for s in range(S)])) for u in range(n)]
        group = oracle_crc(clib(), ctype, data[:logical])
        for a in (t, sums):
            a.setflags(write=False)
        _groups[key] = (t, lens, sums, units, group)
    return _groups[key]


def be32(tensor):
    return [int.from_bytes(bytes(row), "big") for row in tensor.cpu().numpy().reshape(-1, 4).tolist()]


def short_losses(k, m, cell, S, data_len):
    """A data unit before the cut, the one containing it, one past it (length
    0 in the last stripe) and a parity unit, where the group has them; a double
    loss of the cut unit and a parity unit."""
    r = (data_len or S * k * cell) - (S - 1) * k * cell
    cu = (r - 1) // cell  # the data unit that holds the file's last byte
    picks = [(u,) for u in dict.fromkeys([cu - 1, cu, cu + 1]) if 0 <= u < k] + [(k + m - 1,)]
    return picks + [(cu, k)]


@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 1536), (3, 2, 528)])
def test_short_last_stripe_then_composite(dev, k, m, cell, ctype):
    """Every data_len of data_len_cases: the target's true-length sums and the
    sentinel everywhere else, nothing at or past n0 read (0xEE is there); then
    hec_composite_crc_device on the same stream with the same data_len gives
    the oracle's CRC of the lost unit's actual bytes and of the file."""
    n, S, bpc = k + m, 3, 512
    cod = coder(k, m)
    runs = []
    for data_len in data_len_cases(k, cell, S):
        t, lens, sums, units, group = short_group(k, m, cell, S, data_len, ctype)
        for li, lost in enumerate(short_losses(k, m, cell, S, data_len)):
            expected = (None, "sep", "same")[(li + data_len) % 3]
            c = Case(cod, t, sums, [lost] * S, dev, expected=expected, pad=32, ctype=ctype, lens=lens,
                     data_len=data_len)
            c.uniform()
            runs.append((c, units, group, None))
    # a corrupt byte inside a survivor's own bytes of the short stripe, and a
    # corrupt expected sum of its last, short chunk: that flag and no other
    data_len = data_len_cases(k, cell, S)[-1]
    t, lens, sums, units, group = short_group(k, m, cell, S, data_len, ctype)
    assert 0 < lens[S - 1][1] < cell and lens[S - 1][1] % bpc
    for kw in (dict(corrupt=[(S - 1, 1, lens[S - 1][1] - 1)]),
               dict(corrupt_sums=[(S - 1, 1, (lens[S - 1][1] - 1) // bpc)])):
        c = Case(cod, t, sums, [(0,)] * S, dev, expected="sep", ctype=ctype, lens=lens, data_len=data_len, **kw)
        assert c.dirty == {S - 1}
        c.uniform()
        runs.append((c, None, None, None))
    torch.cuda.synchronize()
    for i, (c, units, group, _) in enumerate(runs):
        c.check((c.data_len, c.losts[0], c.expected is not None))
        if units is None:
            continue
        # the survivors' sums beside the reconstructed ones, then the composite
        if c.expected is not c.sums:
            for u in range(n):
                if u not in c.losts[0]:
                    c.sums[:, u] = c.ts[:, u]
        _, unit, grp = H.composite_crc_batch(cod, c.sums, k, cell, ctype, bpc, c.data_len, want=("unit", "group"))
        runs[i] = (c, units, group, (unit, grp))
    torch.cuda.synchronize()
    for c, units, group, out in runs:
        if out is None:
            continue
        got_units, got_group = be32(out[0]), be32(out[1])[0]
        for u in c.losts[0]:
            assert got_units[u] == units[u], (c.data_len, c.losts[0], u)
        assert got_units == list(units), (c.data_len, c.losts[0])
        assert got_group == group, (c.data_len, c.losts[0])


# ---- 5. one pattern per stripe ------------------------------------------------------

def guarded_workspace(cod, S, dev):
    """Exactly the advertised bytes between two guard bands."""
    nbytes = cod.reconstruct_crc_mixed_workspace_size(S)
    buf = torch.full((nbytes + 512,), GUARD, dtype=torch.uint8, device=dev)
    return buf, buf[256:256 + nbytes]


@pytest.mark.parametrize("cell", [9232, 1000])
@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_mixed_every_single_loss_doubles_and_idle_stripes(dev, k, m, cell):
    """2(k+m)+1 stripes: every single-unit loss, two-unit losses with a want of
    one of them, and stripes with nothing lost, which get nothing written; the
    workspace of exactly the advertised size keeps its guard bands."""
    n = k + m
    S = 2 * n + 1
    losts, wants = [], []
    for s in range(S):
        if s < n:
            lost = (s,)
            w = lost
        elif s % 3 == 0:
            lost = w = ()
        else:
            lost = (s % n, (s + 4) % n)
            w = (lost[s % 2],)
        losts.append(lost)
        wants.append(w)
    assert sum(1 for l in losts if not l) >= 2 and sum(1 for l in losts if len(l) == 2) >= 4
    cod = coder(k, m)
    buf, ws = guarded_workspace(cod, S, dev)
    a = mixed_case(cod, k, m, S, cell, losts, dev, wants=wants, expected="same", pad=16)
    a.mixed(workspace=ws)
    b = mixed_case(cod, k, m, S, cell, losts, dev, wants=None, expected=None)
    b.mixed()
    torch.cuda.synchronize()
    a.check("want")
    b.check("all")
    assert bool((buf[:256] == GUARD).all()) and bool((buf[256 + ws.numel():] == GUARD).all())


@pytest.mark.parametrize("cell", [9232, 1000])
def test_mixed_dead_unit_as_null_slot(dev, cell):
    """A unit lost in every stripe has no storage: its slot is NULL.  A NULL
    slot that some stripe has present is an argument error, nothing written."""
    k, m, n = 6, 3, 9
    S = 2 * n + 1
    dead = 4
    losts = [tuple(sorted({dead, s % n})) if s % 2 else (dead,) for s in range(S)]
    cod = coder(k, m)
    c = mixed_case(cod, k, m, S, cell, losts, dev, expected="same")
    c.mixed(null_units=(dead,))
    torch.cuda.synchronize()
    c.check("null slot")
    losts[5] = (2,)  # unit 4 is present in stripe 5
    c = mixed_case(cod, k, m, S, cell, losts, dev, expected="sep")
    with pytest.raises(ValueError):
        c.mixed(null_units=(dead,))
    torch.cuda.synchronize()
    c.no_change()


def test_tensor_helper(dev):
    k, m, n, S, cell = 6, 3, 9, 9, 9232
    losts = [(3,) if s % 2 else (3, s % 3) for s in range(S)]
    c = mixed_case(coder(k, m), k, m, S, cell, losts, dev, expected="same")
    ws = H.reconstruct_sums_batch(coder(k, m), c.cells, [present_mask(n, l) for l in losts], c.sums.view(torch.int32),
                                  expected=c.sums, bad=c.bad)
    assert ws.numel() == coder(k, m).reconstruct_crc_mixed_workspace_size(S)
    torch.cuda.synchronize()
    c.check()


# ---- 6. agreement with hec_reconstruct_crc_device -------------------------------------

@pytest.mark.parametrize("cell", [9232, 1000])
def test_same_sums_and_flags_as_reconstruct_crc(dev, cell):
    """The same inputs through hec_reconstruct_crc_device into a scratch
    output: d_sums and d_bad byte-identical, on a fused and a generic shape."""
    k, m, n, S = 6, 3, 9, 9
    cod = coder(k, m)
    lost = (2, 6)
    c = uniform_case(cod, k, m, S, cell, lost, dev, corrupt_sums=[(1, 0, 0), (7, 5, (cell - 1) // 512)])
    c.uniform()
    ptrs, strides = slots(c.cells)
    shards = [None if i in lost else ptrs[i] for i in range(n)]
    scratch = torch.empty((S, n, cell), dtype=torch.uint8, device=dev)
    optrs, ostrides = slots(scratch)
    sums = torch.full_like(c.sums, SENT)
    bad = torch.zeros_like(c.bad)
    cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, sums.data_ptr(),
                               expected_ptr=c.expected.data_ptr(), bad_ptr=bad.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    assert int(bad.sum()) == 2
    assert torch.equal(c.sums, sums)
    assert torch.equal(c.bad, bad)
    assert torch.equal(c.raw, c.exp_raw)


# ---- 7. argument errors, nothing queued -----------------------------------------------

def test_argument_errors_write_nothing(dev):
    k, m, n, S, cell = 6, 3, 9, 4, 9232
    cod = coder(k, m)
    c = uniform_case(cod, k, m, S, cell, (1, 7), dev)
    ptrs, strides = slots(c.cells)
    shards = [None if i in (1, 7) else ptrs[i] for i in range(n)]
    masks = [present_mask(n, (1, 7))] * S
    ws = torch.empty(cod.reconstruct_crc_mixed_workspace_size(S) + 16, dtype=torch.uint8, device=dev)
    sp, wp, wn = c.sums.data_ptr(), ws.data_ptr(), ws.numel()

    def both(**kw):
        """The same bad argument to both forms."""
        sums_ptr = kw.pop("sums_ptr", sp)
        cl = kw.pop("cell_len", cell)
        with pytest.raises(ValueError):
            cod.reconstruct_sums_device(shards, strides, cl, S, sums_ptr, stream=stream(), **kw)
        with pytest.raises(ValueError):
            cod.reconstruct_sums_device_mixed(ptrs, strides, masks, None, cl, S, sums_ptr, wp, wn, stream=stream(),
                                              **kw)

    both(checksum_type=H.CHECKSUM_NULL)
    both(checksum_type=7)
    both(cell_len=0)
    both(bytes_per_checksum=0)
    both(sums_ptr=None)
    both(sums_ptr=sp + 2)
    both(expected_ptr=c.expected.data_ptr(), bad_ptr=None)
    # data_len out of range: in or before the last stripe but one, past the
    # group, non-zero without stripes
    for S_, data_len in ((S, (S - 1) * k * cell), (S, 1), (S, S * k * cell + 1), (0, 5)):
        with pytest.raises(ValueError):
            cod.reconstruct_sums_device(shards, strides, cell, S_, sp, data_len=data_len, stream=stream())
    # a want bit on a present unit
    with pytest.raises(ValueError):
        cod.reconstruct_sums_device(shards, strides, cell, S, sp, want=[0], stream=stream())
    with pytest.raises(ValueError):
        cod.reconstruct_sums_device_mixed(ptrs, strides, masks, [1 << 7, 1 << 1, 1 << 0, 1 << 7], cell, S, sp, wp, wn,
                                          stream=stream())
    # a target and fewer than k units present
    with pytest.raises(H.ErasureCodingError):
        cod.reconstruct_sums_device([None] * 4 + ptrs[4:], strides, cell, S, sp, stream=stream())
    few = [present_mask(n, (0,)), present_mask(n, ()), present_mask(n, (1, 2, 7, 8)), present_mask(n, (6,))]
    rc = H.lib.hec_reconstruct_sums_device_mixed(cod.handle, C32C, H._pp(ptrs), H._sp(strides),
                                                 (ctypes.c_uint64 * S)(*few), None, cell, S, 512,
                                                 ctypes.c_void_p(c.expected.data_ptr()),
                                                 ctypes.c_void_p(c.bad.data_ptr()), ctypes.c_void_p(sp),
                                                 ctypes.c_void_p(wp), wn, ctypes.c_void_p(stream()))
    assert rc == H.HEC_ERR_NOT_ENOUGH_SHARDS
    # a workspace that is too small, NULL or misaligned
    for p, nbytes in ((wp, cod.reconstruct_mixed_workspace_size(S)), (wp, 64), (None, wn), (wp + 2, wn - 2)):
        with pytest.raises(ValueError):
            cod.reconstruct_sums_device_mixed(ptrs, strides, masks, None, cell, S, sp, p, nbytes, stream=stream())
    torch.cuda.synchronize()
    c.no_change()
    # no stripes, or no target anywhere: OK, and still nothing written
    cod.reconstruct_sums_device(shards, strides, cell, 0, sp, stream=stream())
    cod.reconstruct_sums_device(shards, strides, cell, S, sp, want=[], stream=stream())
    cod.reconstruct_sums_device(ptrs, strides, cell, S, sp, stream=stream())
    cod.reconstruct_sums_device_mixed(ptrs, strides, [], None, cell, 0, sp, wp, wn, stream=stream())
    cod.reconstruct_sums_device_mixed(ptrs, strides, masks, [0] * S, cell, S, sp, wp, wn, stream=stream())
    cod.reconstruct_sums_device_mixed(ptrs, strides, [present_mask(n, ())] * S, None, cell, S, sp, wp, wn,
                                      stream=stream())
    torch.cuda.synchronize()
    c.no_change()


# ---- 8. graph -------------------------------------------------------------------------

def test_graph_capture_replay_with_composite(dev):
    """The uniform call (full stripes through the fused kernel, a short last
    stripe through the generic one) and hec_composite_crc_device captured on
    one stream; replayed, the data changed, replayed again: the sums, the lost
    unit's CRC and the file's CRC follow the data both times."""
    k, m, n, S, cell, bpc = 6, 3, 9, 3, 1536, 512
    data_len = data_len_cases(k, cell, S)[-1]
    cod = coder(k, m)
    lost = (1,)
    ga = short_group(k, m, cell, S, data_len, C32C)
    gb = short_group(k, m, cell, S, data_len, C32C, seed=1)
    c = Case(cod, ga[0], ga[2], [lost] * S, dev, expected="same", lens=ga[1], data_len=data_len)
    other = Case(cod, gb[0], gb[2], [lost] * S, dev, expected="same", lens=gb[1], data_len=data_len)
    unit = torch.zeros((n, 4), dtype=torch.uint8, device=dev)
    grp = torch.zeros((4,), dtype=torch.uint8, device=dev)
    cws = torch.empty(max(4, H.composite_crc_workspace_size(n, S)), dtype=torch.uint8, device=dev)
    first = c.sums.clone()
    c.uniform()  # eager once, then captured
    torch.cuda.synchronize()
    c.check("eager")
    c.sums.copy_(first)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.uniform()
        cod.composite_crc_device(C32C, c.sums.data_ptr(), n, k, cell, S, bpc, data_len, 0, unit.data_ptr(),
                                 grp.data_ptr(), cws.data_ptr(), cws.numel(), stream())
    for rep, (_, _, _, units, group) in enumerate((ga, gb)):
        if rep == 1:  # the other file in the same buffers
            c.raw.copy_(other.raw)
            c.exp_raw.copy_(other.raw)
            c.sums.copy_(other.sums)
            c.exp_sums.copy_(other.exp_sums)
        unit.zero_()
        grp.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.check(("replay", rep))
        assert be32(unit) == list(units), rep
        assert be32(grp)[0] == group, rep
    assert ga[4] != gb[4]
