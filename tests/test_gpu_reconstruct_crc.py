"""Verified reconstruction on the GPU: hec_reconstruct_crc_device (one
pattern per batch) and hec_reconstruct_crc_device_mixed (one per stripe) --
the fused gf_reconstruct_crc kernel and the composed route.  Ground truth is
the stripe that was encoded (random data plus the CPU oracle's parity) and the
C oracle's chunk sums of it, compared as exact bytes.  Every buffer carries
sentinels: 0xEE between cell_len and the stride and in lost slots, 0xA5A5A5A5
in every sums word, zeroed flags; after a call the WHOLE cell buffer, sums
buffer and flags buffer must equal their expected images, so a write to a
present unit, to an unwanted slot, past cell_len or to a sums word of a unit
that was not rebuilt shows as well as a wrong byte."""
import ctypes
import itertools

import numpy as np
import pytest

import ec_oracle as O
import hdfs_native_ec as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GARBAGE = 0xEE
SENT = 0xA5  # every byte of a sums word
# against the kernel's tiles (1-KiB slabs, 4- or 8-KiB wave-tiles, 16- or
# 32-KiB block tiles): one short chunk; a full chunk + a 16-B chunk; a full
# 8-slab wave, then a wave with one slab + a short chunk; 32 KiB + 16 KiB +
# 1 KiB + 16
CELLS = (16, 528, 9232, 50192)
C32C, C32 = H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32


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


def truth(k, m, S, cell, codec="rs"):
    """The original stripes [S, k+m, cell] (computed once per shape, shared,
    read-only): random data and the oracle's parity rows applied to it."""
    key = (k, m, S, cell, codec)
    if key not in _truth:
        rng = np.random.default_rng(7919 * k + 31 * m + S + cell)
        t = np.empty((S, k + m, cell), dtype=np.uint8)
        t[:, :k] = rng.integers(0, 256, size=(S, k, cell), dtype=np.uint8)
        flat = [np.ascontiguousarray(t[:, i]).reshape(-1) for i in range(k)]
        par = O.matmul_shards(O.codec_matrix(codec, k, m)[k:], flat)
        for j in range(m):
            t[:, k + j] = par[j].reshape(S, cell)
        t.setflags(write=False)
        _truth[key] = t
    return _truth[key]


_sums = {}
_clib = None


def chunk_sums(cells, bpc, ctype):
    """The C oracle's chunk sums of cells [..., cell]: uint8 [..., nck, 4]."""
    global _clib
    if _clib is None:
        _clib = O.load_c_oracle()
    cell = cells.shape[-1]
    nck = -(-cell // bpc)
    flat = np.ascontiguousarray(cells).reshape(-1, cell)
    out = np.empty((flat.shape[0], nck, 4), dtype=np.uint8)
    for i in range(flat.shape[0]):
        _clib.orc_chunk_checksum(ctype, flat[i].ctypes.data, cell, bpc, out[i].ctypes.data)
    return out.reshape(cells.shape[:-1] + (nck, 4))


def true_sums(k, m, S, cell, codec="rs", bpc=512, ctype=C32C):
    """Chunk sums of truth(...): [S, k+m, nck, 4], once per shape, read-only."""
    key = (k, m, S, cell, codec, bpc, ctype)
    if key not in _sums:
        s = chunk_sums(truth(k, m, S, cell, codec), bpc, ctype)
        s.setflags(write=False)
        _sums[key] = s
    return _sums[key]


def forget(min_bytes):
    """Drops the cached truths of at least min_bytes of cells, with their sums."""
    for key in [key for key, t in _truth.items() if t.nbytes >= min_bytes]:
        del _truth[key]
        for other in [o for o in _sums if o[:5] == key]:
            del _sums[other]


def patterns(n, lo, hi):
    return [lost for e in range(lo, hi + 1) for lost in itertools.combinations(range(n), e)]


def present_mask(n, lost):
    return ((1 << n) - 1) & ~sum(1 << i for i in lost)


def slots(buf):
    """(ptrs, strides) of the k+m unit slots of a [S, n, width] buffer."""
    S, n, width = buf.shape
    return [buf.data_ptr() + i * width for i in range(n)], [n * width] * n


def stream():
    return torch.cuda.current_stream().cuda_stream


class Case:
    """One call's buffers and their expected images.

    losts[s] = the units stripe s lacks, wants[s] = those to rebuild (None:
    all of them).  corrupt = [(stripe, unit, byte)]: that byte of a present
    cell is flipped; corrupt_sums = [(stripe, unit, chunk)]: that expected sum
    instead.  expected: "sep" = a buffer of its own holding every true sum,
    "same" = the sums buffer itself (true sums at the present units'
    slots), None = no verification.  separate = rebuilt units go to an output
    buffer of their own (filled 0xA5) instead of their slots.  base_off moves
    the cell buffer's base off the 16-B grid."""

    def __init__(self, cod, t, true, losts, dev, wants=None, expected="sep", corrupt=(), corrupt_sums=(), pad=0,
                 separate=False, base_off=0, bpc=512, ctype=C32C):
        S, n, cell = t.shape
        self.cod, self.S, self.n, self.cell, self.bpc, self.ctype = cod, S, n, cell, bpc, ctype
        self.k = cod.data_units
        self.losts = [tuple(l) for l in losts]
        self.wants = [tuple(l) for l in losts] if wants is None else [tuple(w) for w in wants]
        self.have_want = wants is not None
        width = cell + pad
        raw = torch.full((S * n * width + base_off,), GARBAGE, dtype=torch.uint8, device=dev)
        self.cells = raw[base_off:].view(S, n, width)
        self.cells[:, :, :cell] = torch.from_numpy(t.copy()).to(dev)
        for (s, u, b) in corrupt:
            assert u not in self.losts[s]
            self.cells[s, u, b] ^= 0x40
        self.exp_cells = self.cells.clone()  # the corrupt bytes stay where they are
        for s, lost in enumerate(self.losts):
            for i in lost:
                self.cells[s, i] = GARBAGE
                if separate or i not in self.wants[s]:
                    self.exp_cells[s, i] = GARBAGE
        self.out = self.exp_out = None
        if separate:
            self.out = torch.full((S, n, width), 0xA5, dtype=torch.uint8, device=dev)
            self.exp_out = self.out.clone()
            for s, w in enumerate(self.wants):
                for i in w:
                    self.exp_out[s, i, :cell] = torch.from_numpy(t[s, i].copy()).to(dev)
        ts = torch.from_numpy(true.copy()).to(dev)  # [S, n, nck, 4]
        self.sums = torch.full(tuple(ts.shape), SENT, dtype=torch.uint8, device=dev)
        self.expected = None
        if expected == "sep":
            self.expected = ts.clone()
        elif expected == "same":
            for s, lost in enumerate(self.losts):
                keep = [i for i in range(n) if i not in lost]
                self.sums[s, keep] = ts[s, keep]
            self.expected = self.sums
        if expected is not None:
            for (s, u, c) in corrupt_sums:
                assert u not in self.losts[s]
                self.expected[s, u, c, 3] ^= 1
        self.exp_sums = self.sums.clone()
        for s, w in enumerate(self.wants):
            for i in w:
                self.exp_sums[s, i] = ts[s, i]
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

    def ptr_args(self):
        ptrs, strides = slots(self.cells)
        optrs, ostrides = slots(self.out) if self.out is not None else (ptrs, strides)
        return ptrs, strides, optrs, ostrides

    def chk_args(self):
        return dict(expected_ptr=None if self.expected is None else self.expected.data_ptr(),
                    bad_ptr=None if self.expected is None else self.bad.data_ptr(),
                    bytes_per_checksum=self.bpc, checksum_type=self.ctype)

    def uniform(self, strm=None, drop_out=None):
        """One hec_reconstruct_crc_device call: every stripe lacks losts[0]."""
        assert len(set(self.losts)) == 1 and len(set(self.wants)) == 1
        ptrs, strides, optrs, ostrides = self.ptr_args()
        shards = [None if i in self.losts[0] else ptrs[i] for i in range(self.n)]
        if drop_out is not None:
            optrs = [None if i == drop_out else p for i, p in enumerate(optrs)]
        self.cod.reconstruct_crc_device(shards, strides, optrs, ostrides, self.cell, self.S, self.sums.data_ptr(),
                                        want=list(self.wants[0]) if self.have_want else None,
                                        stream=stream() if strm is None else strm, **self.chk_args())

    def mixed(self, workspace=None, strm=None, present=None, wants=None):
        """One hec_reconstruct_crc_device_mixed call (present / wants: masks
        that override those of losts / wants)."""
        ptrs, strides, optrs, ostrides = self.ptr_args()
        masks = present if present is not None else [present_mask(self.n, l) for l in self.losts]
        if wants is None and self.have_want:
            wants = [sum(1 << i for i in w) for w in self.wants]
        if workspace is None:
            workspace = torch.empty(self.cod.reconstruct_crc_mixed_workspace_size(self.S), dtype=torch.uint8,
                                    device=self.cells.device)
        self.workspace = workspace
        self.cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, wants, self.cell, self.S,
                                              self.sums.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                              stream=stream() if strm is None else strm, **self.chk_args())

    def check(self, what=""):
        """After a synchronize: everything equals its expected image; in a
        stripe that read a corrupt survivor the targets and their sums are
        unspecified, everything else still holds."""
        assert torch.equal(self.bad, self.exp_bad), (what, "flags", self.bad.nonzero().tolist(),
                                                     self.exp_bad.nonzero().tolist())
        got = [self.cells, self.sums] + ([self.out] if self.out is not None else [])
        exp = [self.exp_cells, self.exp_sums] + ([self.exp_out] if self.out is not None else [])
        if self.dirty:
            got, exp = [g.clone() for g in got], [e.clone() for e in exp]
            for s in self.dirty:
                for i in self.wants[s]:
                    for g, e in zip(got, exp):
                        g[s, i] = 0
                        e[s, i] = 0
        for name, g, e in zip(("cells", "sums", "out"), got, exp):
            if not torch.equal(g, e):
                diff = (g != e).reshape(g.shape[0], g.shape[1], -1).any(dim=2).nonzero().tolist()
                raise AssertionError((what, name, "stripe/unit pairs that differ", diff[:20]))

    def no_change(self, what=""):
        """Nothing was written: every buffer still holds its initial image."""
        assert not bool(self.bad.any()), what
        assert bool((self.sums == SENT).all()) or self.expected is self.sums, what
        if self.out is not None:
            assert bool((self.out == 0xA5).all()), what
            assert torch.equal(self.cells, self.exp_cells), what


def uniform_case(cod, k, m, S, cell, lost, dev, want=None, codec="rs", **kw):
    bpc, ctype = kw.get("bpc", 512), kw.get("ctype", C32C)
    return Case(cod, truth(k, m, S, cell, codec), true_sums(k, m, S, cell, codec, bpc, ctype), [lost] * S, dev,
                wants=None if want is None else [want] * S, **kw)


def mixed_case(cod, k, m, S, cell, losts, dev, wants=None, codec="rs", **kw):
    bpc, ctype = kw.get("bpc", 512), kw.get("ctype", C32C)
    return Case(cod, truth(k, m, S, cell, codec), true_sums(k, m, S, cell, codec, bpc, ctype), losts, dev,
                wants=wants, **kw)


# ---- 1. one pattern per batch, every pattern ------------------------------------

@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("cell", CELLS)
def test_uniform_rs63_every_pattern_in_place(dev, cell, S):
    """RS(6,3), all 129 patterns of 1..3 lost units, each on its own copy of
    the batch, in place, CRC32C, verified against the true sums (no flag may be
    set).  In half of the parametrisations d_expected is d_sums itself: the
    call fills the holes of one sums array."""
    k, m, n = 6, 3, 9
    pats = patterns(n, 1, m)
    assert len(pats) == 129
    same = (CELLS.index(cell) + (S == 9)) % 2 == 1
    P = len(pats)
    want = torch.from_numpy(truth(k, m, S, cell).copy()).to(dev)
    ts = torch.from_numpy(true_sums(k, m, S, cell).copy()).to(dev)
    bufs = want.unsqueeze(0).repeat(P, 1, 1, 1)
    sums = torch.full((P,) + tuple(ts.shape), SENT, dtype=torch.uint8, device=dev)
    exp_sums = sums.clone()
    if same:
        sums[:] = ts
        exp_sums[:] = ts
    bad = torch.zeros((P, S, n), dtype=torch.uint8, device=dev)
    for p, lost in enumerate(pats):
        for i in lost:
            bufs[p, :, i] = GARBAGE
            sums[p, :, i] = SENT
            exp_sums[p, :, i] = ts[:, i]
    for p, lost in enumerate(pats):
        ptrs, strides = slots(bufs[p])
        coder(k, m).reconstruct_crc_device([None if i in lost else ptrs[i] for i in range(n)], strides, ptrs, strides,
                                           cell, S, sums[p].data_ptr(),
                                           expected_ptr=(sums[p] if same else ts).data_ptr(),
                                           bad_ptr=bad[p].data_ptr(), stream=stream())
    torch.cuda.synchronize()
    ok_cells = (bufs == want.unsqueeze(0)).reshape(P, -1).all(dim=1)
    ok_sums = (sums == exp_sums).reshape(P, -1).all(dim=1)
    wrong = [pats[p] for p in range(P) if not (bool(ok_cells[p]) and bool(ok_sums[p]))]
    assert not wrong, wrong
    assert not bool(bad.any()), [pats[p] for p in bad.reshape(P, -1).any(dim=1).nonzero().flatten().tolist()]


# ---- 2. other shapes ------------------------------------------------------------

def _sample(n, m, count, seed, extra):
    pats = patterns(n, 1, m)
    rng = np.random.default_rng(seed)
    return [pats[i] for i in rng.choice(len(pats), size=count, replace=False)] + list(extra)


@pytest.mark.parametrize("ctype", [C32C, C32])
@pytest.mark.parametrize("k,m,cell", [(2, 1, 9232), (3, 2, 9232), (10, 4, 528), (10, 4, 50192)])
def test_uniform_other_shapes_separate_outputs(dev, k, m, cell, ctype):
    """RS(2,1) and RS(3,2), every pattern, and RS(10,4), a fixed sample that
    includes 4 units lost with parity among them, into output buffers of
    their own, both checksum types."""
    n, S = k + m, 9 if cell < 50000 else 3
    if k <= 3:
        picks = patterns(n, 1, m)  # all 3 / all 15
    else:
        picks = _sample(n, m, 12, 1040 + cell, [(10, 11, 12, 13), (0, 5, 9, 12), (3, 13)])
    cases = [uniform_case(coder(k, m), k, m, S, cell, lost, dev, separate=True, pad=48, ctype=ctype) for lost in picks]
    for c in cases:
        c.uniform()
    torch.cuda.synchronize()
    for lost, c in zip(picks, cases):
        c.check(lost)


def test_uniform_rs_legacy(dev):
    k, m, S, cell = 6, 3, 9, 9232
    c = uniform_case(coder(k, m, "rs-legacy"), k, m, S, cell, (1, 7), dev, codec="rs-legacy")
    c.uniform()
    torch.cuda.synchronize()
    c.check()


@pytest.mark.parametrize("ctype", [C32C, C32])
def test_uniform_want_narrows_to_one_unit(dev, ctype):
    """Two units lost, one wanted: the other slot and its sums keep their sentinels."""
    k, m, S, cell = 6, 3, 9, 9232
    for lost, want in [((1, 7), (7,)), ((1, 7), (1,)), ((0, 4, 8), (4,))]:
        c = uniform_case(coder(k, m), k, m, S, cell, lost, dev, want=want, ctype=ctype, pad=16)
        c.uniform()
        torch.cuda.synchronize()
        c.check((lost, want))


# ---- 3. without d_expected ------------------------------------------------------

@pytest.mark.parametrize("cell", [528, 9232])
def test_uniform_without_expected(dev, cell):
    """d_expected = d_bad = NULL: the same bytes and sums, nothing verified."""
    k, m, S = 6, 3, 9
    picks = [(0,), (5,), (6,), (8,), (0, 1), (2, 7), (7, 8), (0, 1, 2), (3, 6, 8), (6, 7, 8)]
    cases = [uniform_case(coder(k, m), k, m, S, cell, lost, dev, expected=None) for lost in picks]
    for c in cases:
        c.uniform()
    torch.cuda.synchronize()
    for lost, c in zip(picks, cases):
        c.check(lost)
    # a corrupt survivor goes unnoticed: the call is OK and flags nothing
    c = uniform_case(coder(k, m), k, m, S, cell, (2,), dev, expected=None, corrupt=[(4, 0, 17)])
    c.uniform()
    torch.cuda.synchronize()
    assert c.dirty == {4} and not bool(c.bad.any())
    c.check()


KERNEL_SHAPES = [(k, r) for k in (2, 3, 6, 10) for r in (1, 2, 3, 4)]


@pytest.mark.parametrize("k,r", KERNEL_SHAPES, ids=[f"k{k}-r{r}" for k, r in KERNEL_SHAPES])
def test_every_kernel_shape(dev, k, r):
    """gf_reconstruct_crc<K, R, .., KIND, VERIFY_IN> at every (K, R) it is built
    for, both checksum types, with and without d_expected: RS(k,4) with r units
    lost, data and parity among them.  528 B = one full chunk and a 16-B short
    one, 9232 B = a short last tile; with d_expected a survivor of stripe 1 has
    a corrupt byte in its last 16 B and must be the one flag."""
    m, S = 4, 3
    lost = tuple(range(k - (r + 1) // 2, k + r // 2))  # the last data units and the first parity units
    surv = [i for i in range(k + m) if i not in lost][:k]
    cases = []
    for cell in (528, 9232):
        for ctype in (C32C, C32):
            cases.append(uniform_case(coder(k, m), k, m, S, cell, lost, dev, ctype=ctype,
                                      corrupt=[(1, surv[-1], cell - 5)]))
            cases.append(uniform_case(coder(k, m), k, m, S, cell, lost, dev, ctype=ctype, expected=None))
    for c in cases:
        c.uniform()
    torch.cuda.synchronize()
    for c in cases:
        assert c.dirty == ({1} if c.expected is not None else set())
        c.check((c.cell, c.ctype, c.expected is not None))


# ---- 4. verification ------------------------------------------------------------

@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("k,m,cell", [(6, 3, 9232), (6, 3, 50192), (10, 4, 9232)])
def test_verification_flags_exactly_the_corrupt_survivors(dev, k, m, cell, form):
    """One flipped byte in a survivor cell of chosen stripes: the first chunk,
    a middle chunk, the short last chunk, the last byte of a full chunk, and a
    present unit the plan does not read (never flagged).  Then the same cells
    through a wrong expected sum instead of wrong data."""
    n, S = k + m, 9
    lost = (1,)  # survivors: 0, 2 .. k; units k+1 .. are present and unread
    nck = -(-cell // 512)
    spots = [(0, 0, 0), (2, 2, (nck // 2) * 512 + 100), (3, k, cell - 1), (5, 3, 511), (7, n - 1, 40),
             (8, 0, cell - 17), (8, 4, 1024 + 5)]
    for by_sum in (False, True):
        if by_sum:
            kw = dict(corrupt_sums=[(s, u, b // 512) for (s, u, b) in spots])
        else:
            kw = dict(corrupt=spots)
        c = uniform_case(coder(k, m), k, m, S, cell, lost, dev, **kw)
        assert c.dirty == {0, 2, 3, 5, 8} and int(c.exp_bad.sum()) == 6
        c.uniform() if form == "uniform" else c.mixed()
        torch.cuda.synchronize()
        c.check((form, by_sum))


# ---- 5. one pattern per stripe --------------------------------------------------

@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
@pytest.mark.parametrize("cell", CELLS)
def test_mixed_node_failure_and_random(dev, k, m, cell):
    """S = 37.  One lost unit per stripe with the index uniform over k+m (a
    dead node's block groups), in place; then random 0..m losses with a random
    non-empty want (stripes with nothing lost keep everything untouched)."""
    n, S = k + m, 37
    rng = np.random.default_rng(37 * k + cell)
    losts = [(int(rng.integers(0, n)),) for _ in range(S)]
    a = mixed_case(coder(k, m), k, m, S, cell, losts, dev, expected="same")
    a.mixed()
    losts, wants = [], []
    for s in range(S):
        e = int(rng.integers(0, m + 1)) if s else 0  # stripe 0: nothing lost
        lost = tuple(sorted(rng.choice(n, size=e, replace=False).tolist()))
        w = tuple(i for i in lost if rng.integers(0, 2))
        losts.append(lost)
        wants.append(w if w or not lost else lost[:1])
    b = mixed_case(coder(k, m), k, m, S, cell, losts, dev, wants=wants, pad=32)
    b.mixed()
    torch.cuda.synchronize()
    a.check("node failure")
    b.check("random")


# ---- 6. flag, re-plan, repair ---------------------------------------------------

def test_flag_replan_repair(dev):
    """RS(6,3), one lost unit per stripe and a corrupt survivor in 3 stripes:
    the first mixed call flags them, the second runs only on the flagged
    stripes with the bad unit cleared from present and added to want; the
    cells then equal the truth everywhere and every rebuilt unit has the
    oracle's sums."""
    k, m, n, S, cell = 6, 3, 9, 9, 9232
    t, ts = truth(k, m, S, cell), true_sums(k, m, S, cell)
    losts = [((2 * s + 1) % n,) for s in range(S)]
    corrupt = [(1, 0, 5), (4, 2, 9000), (6, 5, 9231)]
    for (s, u, _) in corrupt:
        assert u not in losts[s] and u in [i for i in range(n) if i not in losts[s]][:k]
    c = mixed_case(coder(k, m), k, m, S, cell, losts, dev, corrupt=corrupt, expected="same")
    c.mixed()
    torch.cuda.synchronize()
    c.check("first pass")
    bad = c.bad.cpu().numpy()
    assert sorted(np.argwhere(bad).tolist()) == sorted([s, u] for (s, u, _) in corrupt)
    present, want = [], []
    for s in range(S):
        mask = present_mask(n, losts[s])
        w = 0
        if bad[s].any():
            badmask = sum(1 << int(u) for u in np.flatnonzero(bad[s]))
            mask &= ~badmask
            w = badmask | (1 << losts[s][0])
        present.append(mask)
        want.append(w)
    c.bad.zero_()
    c.mixed(present=present, wants=want)
    torch.cuda.synchronize()
    assert not bool(c.bad.any())
    assert torch.equal(c.cells, torch.from_numpy(t.copy()).to(dev))
    got = c.sums.cpu().numpy()
    for s in range(S):
        rebuilt = set(losts[s]) | {u for (cs, u, _) in corrupt if cs == s}
        for i in rebuilt:
            assert np.array_equal(got[s, i], ts[s, i]), (s, i)


# ---- 7. the composed route --------------------------------------------------------

@pytest.mark.parametrize("form", ["uniform", "mixed"])
@pytest.mark.parametrize("shape", ["cell1000", "cell37", "bpc256", "bpc4096", "rs42", "xor51", "rs66", "base8"])
def test_composed_route_same_results(dev, shape, form):
    """The shapes the fused kernel does not take run a verify pass, the plain
    reconstruct call and a checksum pass: same bytes, sums and flags."""
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
        k, m, lost = 4, 2, (0, 5)
    elif shape == "xor51":
        k, m, codec, lost = 5, 1, "xor", (3,)
    elif shape == "rs66":
        k, m, lost = 6, 6, (0, 2, 7, 9, 11)  # 5 target rows
    elif shape == "base8":
        kw["base_off"] = 8
    n, S = k + m, 9
    cod = coder(k, m, codec)
    surv = [i for i in range(n) if i not in lost][:k]
    corrupt = [(3, surv[0], cell // 2), (5, surv[-1], cell - 1)]
    if form == "uniform":
        a = uniform_case(cod, k, m, S, cell, lost, dev, codec=codec, **kw)
        b = uniform_case(cod, k, m, S, cell, lost, dev, codec=codec, corrupt=corrupt, expected="same", **kw)
        a.uniform()
        b.uniform()
    else:
        pats = [()] + [p for p in patterns(n, 1, min(m, 2))] + [lost]
        losts = [pats[(5 * s + 1) % len(pats)] for s in range(S - 1)] + [lost]
        a = mixed_case(cod, k, m, S, cell, losts, dev, codec=codec, **kw)
        losts_b = [lost] * S
        b = mixed_case(cod, k, m, S, cell, losts_b, dev, codec=codec, corrupt=corrupt, expected="same", **kw)
        a.mixed()
        b.mixed()
    if shape == "base8":
        assert a.cells.data_ptr() % 16 == 8
    torch.cuda.synchronize()
    a.check((shape, form, "clean"))
    assert b.dirty == {3, 5}
    b.check((shape, form, "corrupt"))


# ---- 8. capture and streams -----------------------------------------------------

def test_graph_capture_replay(dev):
    """One eager uniform call, then the same call captured on a side stream
    (the launch takes no counters: nothing else is in the graph); targets and
    sums scribbled over, replayed, exact again."""
    k, m, S, cell = 6, 3, 9, 50192
    c = uniform_case(coder(k, m), k, m, S, cell, (0, 8), dev)
    c.uniform()
    torch.cuda.synchronize()
    c.check("eager")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c.uniform()
    for rep in range(2):
        for i in (0, 8):
            c.cells[:, i] = GARBAGE
            c.sums[:, i] = SENT
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        c.check(("replay", rep))


def test_two_mixed_calls_on_two_streams(dev):
    """Two mixed calls in flight on two streams, each with its own workspace."""
    k, m, n, S, cell = 6, 3, 9, 37, 50192
    rng = np.random.default_rng(2)
    cases = []
    for call in range(2):
        losts = [(int(rng.integers(0, n)),) for _ in range(S)]
        cases.append(mixed_case(coder(k, m), k, m, S, cell, losts, dev, expected="same"))
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    for c, st in zip(cases, streams):
        ws = torch.empty(coder(k, m).reconstruct_crc_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
        with torch.cuda.stream(st):
            c.mixed(workspace=ws)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        c.check(i)


# ---- 9. argument errors ---------------------------------------------------------

def test_argument_errors_write_nothing(dev):
    k, m, n, S, cell = 6, 3, 9, 4, 9232
    cod = coder(k, m)
    # d_expected without d_bad
    c = uniform_case(cod, k, m, S, cell, (1, 7), dev, separate=True)
    ptrs, strides, optrs, ostrides = c.ptr_args()
    shards = [None if i in (1, 7) else ptrs[i] for i in range(n)]
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, c.sums.data_ptr(),
                                   expected_ptr=c.expected.data_ptr(), bad_ptr=None, stream=stream())
    ws = torch.empty(cod.reconstruct_crc_mixed_workspace_size(S), dtype=torch.uint8, device=dev)
    masks = [present_mask(n, (1, 7))] * S
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, None, cell, S, c.sums.data_ptr(),
                                         ws.data_ptr(), ws.numel(), expected_ptr=c.expected.data_ptr(),
                                         bad_ptr=None, stream=stream())
    # a misaligned d_sums, a NULL d_sums
    for sums_ptr in (c.sums.data_ptr() + 2, None):
        with pytest.raises(ValueError):
            cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, sums_ptr, stream=stream())
        with pytest.raises(ValueError):
            cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, None, cell, S, sums_ptr,
                                             ws.data_ptr(), ws.numel(), stream=stream())
    # bytes_per_checksum == 0
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, c.sums.data_ptr(),
                                   bytes_per_checksum=0, stream=stream())
    # a NULL d_out at a target
    with pytest.raises(ValueError):
        c.uniform(drop_out=7)
    no7 = [None if i == 7 else p for i, p in enumerate(optrs)]
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device_mixed(ptrs, strides, no7, ostrides, masks, None, cell, S, c.sums.data_ptr(),
                                         ws.data_ptr(), ws.numel(), bad_ptr=c.bad.data_ptr(),
                                         expected_ptr=c.expected.data_ptr(), stream=stream())
    # a want bit on a present unit
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, c.sums.data_ptr(), want=[0],
                                   stream=stream())
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, [1 << 7, 1 << 1, 1 << 0, 1 << 7],
                                         cell, S, c.sums.data_ptr(), ws.data_ptr(), ws.numel(), stream=stream())
    # a target and fewer than k units present
    with pytest.raises(H.ErasureCodingError):
        cod.reconstruct_crc_device([None] * 4 + ptrs[4:], strides, optrs, ostrides, cell, S, c.sums.data_ptr(),
                                   stream=stream())
    few = [present_mask(n, (0,)), present_mask(n, ()), present_mask(n, (1, 2, 7, 8)), present_mask(n, (6,))]
    rc = H.lib.hec_reconstruct_crc_device_mixed(cod.handle, C32C, H._pp(ptrs), H._sp(strides), H._pp(optrs),
                                                H._sp(ostrides), (ctypes.c_uint64 * S)(*few), None, cell, S, 512,
                                                ctypes.c_void_p(c.expected.data_ptr()),
                                                ctypes.c_void_p(c.bad.data_ptr()),
                                                ctypes.c_void_p(c.sums.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                                ws.numel(), ctypes.c_void_p(stream()))
    assert rc == H.HEC_ERR_NOT_ENOUGH_SHARDS
    # a workspace too small for the lists
    with pytest.raises(ValueError):
        cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, None, cell, S, c.sums.data_ptr(),
                                         ws.data_ptr(), cod.reconstruct_mixed_workspace_size(S), stream=stream())
    torch.cuda.synchronize()
    c.no_change()
    # nothing wanted, or no stripes: OK, and still nothing written
    cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, S, c.sums.data_ptr(), want=[], stream=stream())
    cod.reconstruct_crc_device_mixed(ptrs, strides, optrs, ostrides, masks, [0] * S, cell, S, c.sums.data_ptr(),
                                     ws.data_ptr(), ws.numel(), stream=stream())
    cod.reconstruct_crc_device(shards, strides, optrs, ostrides, cell, 0, c.sums.data_ptr(), stream=stream())
    torch.cuda.synchronize()
    c.no_change()


def test_checksum_null_is_the_plain_call(dev):
    """HEC_CHECKSUM_NULL: the plain reconstruct; the checksum buffers are ignored."""
    k, m, S, cell = 6, 3, 9, 9232
    c = uniform_case(coder(k, m), k, m, S, cell, (2, 6), dev, ctype=H.CHECKSUM_NULL, corrupt_sums=[(1, 0, 0)])
    c.exp_sums[:] = SENT
    c.exp_bad.zero_()
    c.dirty = set()
    c.uniform()
    torch.cuda.synchronize()
    c.check()


def test_tensor_helper(dev):
    k, m, n, S, cell = 6, 3, 9, 9, 9232
    losts = [(s % n,) for s in range(S)]
    c = mixed_case(coder(k, m), k, m, S, cell, losts, dev, expected="same")
    ws = H.reconstruct_crc_batch_mixed(coder(k, m), c.cells, [present_mask(n, l) for l in losts],
                                       c.sums.view(torch.int32), expected=c.sums, bad=c.bad)
    assert ws.numel() == coder(k, m).reconstruct_crc_mixed_workspace_size(S)
    torch.cuda.synchronize()
    c.check()
