"""The fused coding + checksum kernel gf_fused_crc (csrc/ec_fused_kernel.hpp,
dispatched by launch_fused in csrc/ec_fused.hip, specialised per decode plan by
csrc/jit.cpp) behind hec_encode_crc_device and hec_decode_verify_device, pinned
the way test_gpu_coding_launch.py pins the plain coding launch:

  1. every instantiation the product library compiles, at the smallest cells
     that reach every branch of a tile (fused_launch_cases.py): encode + CRC at
     all 16 (k, m) of the RS matrix, with the rs-legacy and xor matrices (the
     v_perm form at shapes that otherwise run the bit-sliced one) and at five
     shapes the fused launch refuses; the generic decode + verify kernel in a
     child process with HEC_JIT=0 (fused_generic_child.py), which is the only
     way to be sure the generic kernel ran; the plan-specialised kernel after a
     synchronous prepare_decode, with the launch counter as proof;
  2. launches in which a wave or a block must take several tiles: the
     work-queue kernels at tile counts up to 3 W + 5 for W resident waves, the
     block-tile kernels on the measurement build with a grid of 1 and 5 blocks;
  3. fused launches large and tiny, with a plain coding launch between them,
     back to back on one stream (both counter sets of the stream, DESIGN.md
     §3.1), then captured into a graph and replayed twice.

The reference is the oracle throughout (fused_launch_cases.py: orc_encode_batch,
orc_decode, orc_chunk_checksum, the verified read restated over them), never
another device kernel.  For rs-legacy and xor the matrix comes from
hec_gen_codec_matrix and the product from ec_oracle.matmul_shards: that pins
the kernel against the matrix it is given, not the matrix itself
(test_gpu_parity.py::test_rs_legacy_codec_encode_decode does that).

Every buffer is compared as a whole image: rows have a pitch of cell + 64,
outputs start as 0xA5, input gaps and the slots of lost units hold 0xEE, the
sums array and the flags have a band of 0xC3 in front and behind, d_bad starts
as 7.  After a run every output buffer equals its expected image -- pitch gaps
and a decode's present and verified units still 0xA5 --, every word outside the
call keeps its fill and every input buffer is unchanged."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fused_launch_cases as C
import hdfs_native_ec as H
from test_gpu_coding_launch import BAND, GARBAGE, SENT, Rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
BAND_BYTES = 256
needs_measurement_build = pytest.mark.skipif(not H.experimental_available(),
                                             reason="measurement build not built (make -C hdfs-native_amd exp)")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_coders = {}


def coder(k, m, codec="rs", lib=None):
    key = (k, m, codec, id(lib))
    if key not in _coders:
        _coders[key] = H.Coder(k, m, 0, codec, lib=lib)
    return _coders[key]


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def jit_launches(lib=None):
    if lib is None:
        return H.jit_stats()["launches"]
    v = [ctypes.c_uint64(0) for _ in range(4)]
    lib.hec_jit_stats(*[ctypes.byref(x) for x in v])
    return v[3].value


class Banded:
    """A dense device array (the chunk sums, the flags) between two bands of
    0xC3 and its host image: what upload() puts there or what a run must leave."""

    def __init__(self, dev, shape, fill):
        self.fill = fill
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * BAND_BYTES,), BAND, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw[BAND_BYTES:BAND_BYTES + n].view(*shape)
        self.image = np.full(shape, fill, dtype=np.uint8)

    def ptr(self):
        return self.view.data_ptr()

    def upload(self):
        self.view.copy_(torch.from_numpy(self.image))

    def clear(self):
        self.view.fill_(self.fill)

    def check(self, what, rows=None):
        """rows: the leading indices that are compared (default: all)."""
        bands = torch.cat([self.raw[:BAND_BYTES], self.raw[-BAND_BYTES:]])
        assert bool((bands == BAND).all()), (what, "band overwritten at", (bands != BAND).nonzero()[:8].tolist())
        got, exp = self.view.cpu().numpy(), self.image
        if rows is not None:
            got, exp = got[rows], exp[rows]
        if not np.array_equal(got, exp):
            ne = np.argwhere(got != exp)
            raise AssertionError((what, "differs at", ne[:8].tolist(), "of", len(ne), "got",
                                  [int(got[tuple(i)]) for i in ne[:8]], "want", [int(exp[tuple(i)]) for i in ne[:8]]))


def parity_ref(codec, k, m, data):
    if codec == "rs":
        return C.encode_ref(k, m, data)
    return C.matrix_parity(H.gen_codec_matrix(codec, k, m)[k:], data)


class EncodeRun:
    """hec_encode_crc_device over one batch: parity rows and the sums array
    against the oracle's parity and the chunk sums of all k + m units."""

    def __init__(self, dev, codec, k, m, stripes, cell, seed, bpc=C.BPC, data_off=0, lib=None, tag="", twin_of=None):
        self.codec, self.k, self.m, self.S, self.cell, self.bpc, self.tag = codec, k, m, stripes, cell, bpc, tag
        self.cod = coder(k, m, codec, lib)
        nck = -(-cell // bpc)
        self.par = Rows(dev, stripes, m, cell, SENT)
        self.sums = Banded(dev, (stripes, k + m, nck, 4), SENT)
        if twin_of is not None:  # the same inputs and truth, outputs of its own
            self.data = twin_of.data
            self.par.image[...] = twin_of.par.image
            self.sums.image[...] = twin_of.sums.image
            return
        self.data = Rows(dev, stripes, k, cell, GARBAGE, base_off=data_off)
        data = C.batch_data(k, stripes, cell, seed)
        par = parity_ref(codec, k, m, data)
        self.data.expect(data)
        self.data.upload()
        self.par.expect(par)
        self.sums.image[...] = C.chunk_sums(np.concatenate([data, par], axis=1), C.CRC32C, bpc)

    def twin(self, dev):
        return EncodeRun(dev, self.codec, self.k, self.m, self.S, self.cell, 0, self.bpc, tag=self.tag + "'",
                         twin_of=self)

    def clear(self):
        self.par.clear()
        self.sums.clear()

    def launch(self, stream):
        self.cod.encode_crc_device(self.data.ptrs(), self.data.strides(), self.par.ptrs(), self.par.strides(),
                                   self.cell, self.S, self.bpc, self.sums.ptr(), stream)

    def check(self, what=""):
        what = (what, "encode + CRC", self.codec, self.k, self.m, "stripes", self.S, "cell", self.cell, self.tag)
        self.par.check(what + ("parity",))
        self.sums.check(what + ("sums [stripe, unit, chunk, byte]",))
        self.data.check(what + ("data changed",))


class PlainRun:
    """hec_encode_device over one batch (a plain coding launch between fused ones)."""

    def __init__(self, dev, k, m, stripes, cell, seed):
        self.k, self.m, self.S, self.cell = k, m, stripes, cell
        self.data = Rows(dev, stripes, k, cell, GARBAGE)
        self.par = Rows(dev, stripes, m, cell, SENT)
        data = C.batch_data(k, stripes, cell, seed)
        self.data.expect(data)
        self.data.upload()
        self.par.expect(C.encode_ref(k, m, data))

    def twin(self, dev):
        other = PlainRun.__new__(PlainRun)
        other.k, other.m, other.S, other.cell, other.data = self.k, self.m, self.S, self.cell, self.data
        other.par = Rows(dev, self.S, self.m, self.cell, SENT)
        other.par.image[...] = self.par.image
        return other

    def clear(self):
        self.par.clear()

    def launch(self, stream):
        coder(self.k, self.m).encode_device(self.data.ptrs(), self.data.strides(), self.par.ptrs(),
                                            self.par.strides(), self.cell, self.S, stream)

    def check(self, what=""):
        what = (what, "plain encode", self.k, self.m, "stripes", self.S, "cell", self.cell)
        self.par.check(what + ("parity",))
        self.data.check(what + ("data changed",))


class VerifyRun:
    """hec_decode_verify_device over the batch of a verify case
    (fused_launch_cases.VerifyTruth): rebuilt cells, flags, the error."""

    def __init__(self, dev, case, cell, seed, stripes=C.VERIFY_STRIPES, flips=None, lib=None):
        k, n = case.k, case.k + case.m
        self.case, self.cell, self.S = case, cell, stripes
        self.cod = coder(k, case.m, "rs", lib)
        t = self.truth = C.VerifyTruth(case, cell, seed, stripes, flips, GARBAGE)
        self.inp = Rows(dev, stripes, n, cell, GARBAGE)
        self.inp.expect(t.units)
        self.inp.upload()
        self.out = Rows(dev, stripes, k, cell, SENT)
        for (s, i), want in t.out.items():
            self.out.image[s, i, :cell] = want
        self.sums = Banded(dev, t.sums.shape, GARBAGE)
        self.sums.image[...] = t.sums
        self.sums.upload()
        self.bad = Banded(dev, (stripes, n), 7)
        self.bad.image[...] = t.bad
        self.lost = set(case.lost_data) | {k + j for j in case.lost_parity}

    def run(self, stream, what=""):
        case, t = self.case, self.truth
        self.out.clear()
        self.bad.clear()
        torch.cuda.synchronize()
        ptrs = [None if i in self.lost else p for i, p in enumerate(self.inp.ptrs())]
        try:
            self.cod.decode_verify_device(case.ctype, ptrs, self.inp.strides(), self.out.ptrs(), self.out.strides(),
                                          self.cell, self.S, C.BPC, self.sums.ptr(), self.bad.ptr(), stream)
            raised = False
        except H.ErasureCodingError:
            raised = True
        torch.cuda.synchronize()
        what = (what, "decode + verify", case.name, "stripes", self.S, "cell", self.cell, "bent", t.flips[:4])
        assert raised == t.raises, what + ("raised", raised)
        self.bad.check(what + ("flags [stripe, unit]",), rows=np.nonzero(t.flags_checked)[0])
        self.out.check(what + ("rebuilt",), free=t.free)
        self.inp.check(what + ("inputs changed",))
        self.sums.check(what + ("expected sums changed",))


def on_side_stream(run, what=""):
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    run.clear()
    run.launch(st.cuda_stream)
    st.synchronize()
    run.check(what)


# ---- 1. every product instantiation, smallest shapes --------------------------------------

@pytest.mark.parametrize("case", C.encode_cases(), ids=lambda c: c.name)
def test_encode_crc_every_instantiation(dev, case):
    """gf_fused_crc<K, R, ...> encode at every (K, R) the product compiles: the
    RS matrix (RsNet where a network exists; the work queue at RS(3,2) and
    RS(10,4)), and the rs-legacy and xor matrices (PermNet)."""
    for x, cell in enumerate(case.cells):
        on_side_stream(EncodeRun(dev, case.codec, case.k, case.m, C.STRIPES, cell, seed=1000 + 7 * x + case.k))


@pytest.mark.parametrize("case", C.fallback_cases(), ids=lambda c: c.name)
def test_encode_crc_fallback_shapes(dev, case):
    """Shapes the fused launch refuses: a plain encode and a checksum pass must
    leave the same images."""
    for cell in case.cells:
        run = EncodeRun(dev, case.codec, case.k, case.m, C.STRIPES, cell, seed=2000 + case.k, bpc=case.bpc,
                        data_off=case.data_off)
        if case.data_off:
            assert all(p % 16 == case.data_off for p in run.data.ptrs())
        on_side_stream(run)


def run_verify_case(dev, case, seed0, lib=None):
    st = torch.cuda.Stream()
    for x, cell in enumerate(case.cells):
        VerifyRun(dev, case, cell, seed=seed0 + x, lib=lib).run(st.cuda_stream)


@pytest.fixture(scope="module")
def generic_verdicts():
    """fused_generic_child.py, once: {case name: verdict} and its last line."""
    env = dict(os.environ, HEC_JIT="0")
    child = subprocess.run([sys.executable, os.path.join(HERE, "fused_generic_child.py")], capture_output=True,
                           text=True, timeout=300, env=env)
    lines = [json.loads(line) for line in child.stdout.splitlines() if line.startswith("{")]
    return child, {v["case"]: v for v in lines if "case" in v}, [v for v in lines if "done" in v]


@pytest.mark.parametrize("case", C.generic_cases(), ids=lambda c: c.name)
def test_decode_verify_generic_kernel(generic_verdicts, case):
    """The ahead-of-time decode + verify kernel gf_fused_crc<K, E, SLABS, 12,
    KIND, true, 2, SLABS == 4> at every reachable (K, E) and both checksum
    types, in a process that never specialises (HEC_JIT=0)."""
    child, verdicts, _ = generic_verdicts
    assert case.name in verdicts, (child.returncode, child.stdout[-1500:], child.stderr[-3000:])
    assert verdicts[case.name]["ok"], verdicts[case.name]


def test_decode_verify_generic_child_ran_no_specialised_kernel(generic_verdicts):
    child, verdicts, done = generic_verdicts
    assert child.returncode == 0, (child.returncode, child.stdout[-1500:], child.stderr[-3000:])
    assert len(done) == 1 and done[0] == {"done": True, "cases": len(C.generic_cases()), "jit_launches": 0,
                                          "fixed_order": True}, done
    assert set(verdicts) == {c.name for c in C.generic_cases()}


@pytest.mark.parametrize("case", C.specialised_cases(), ids=lambda c: c.name)
def test_decode_verify_specialised_kernel(dev, case):
    """The plan's own kernel (jit_plan::Net), compiled before the call: every
    call of the case must count as a specialised launch."""
    cod = coder(case.k, case.m)
    lost = list(case.lost_data) + [case.k + j for j in case.lost_parity]
    assert cod.prepare_decode(lost, case.ctype), "hiprtc unavailable on the GPU box"
    before = jit_launches()
    run_verify_case(dev, case, seed0=3000 + 10 * case.k + case.e)
    assert jit_launches() - before == len(case.cells)


# ---- 2. waves and blocks that must take several tiles --------------------------------------

@pytest.mark.parametrize("name", C.QUEUE_T)
@pytest.mark.parametrize("call,k,m,e,wave_tile", C.QUEUE_KERNELS, ids=lambda v: str(v))
def test_queue_kernels_take_several_tiles(dev, call, k, m, e, wave_tile, name):
    """W = 8 x CUs waves are resident in a work-queue launch, so T > j W tiles
    make some wave take j + 1: accumulators set up again, the LDS stage image
    reused, waves past the end of a short tile going on to the next.  The wave
    tile (8 KiB for the 8-slab encode of RS(3,2), 4 KiB for RS(10,4) and for
    jit::default_slabs) is restated in fused_launch_cases.QUEUE_KERNELS: the
    library does not report it.  A change of either slab count has to change
    that list, or T tiles here become another count there."""
    T = dict(C.queue_tile_counts(cu_count()))[name]
    S, cell = C.queue_shape(T, wave_tile)
    assert C.fused_tiles(S, cell, wave_tile) == T
    if call == "encode":
        on_side_stream(EncodeRun(dev, "rs", k, m, S, cell, seed=4000 + T + k, tag="T " + name))
        return
    case = C.VerifyCase(k, m, e, C.CRC32C, C.lost_units(k, e), (), (cell,), "queue-%d-%d-e%d-T%s" % (k, m, e, name))
    lost = list(case.lost_data)
    assert coder(k, m).prepare_decode(lost, case.ctype), "hiprtc unavailable on the GPU box"
    assert C.spares(case) == 0  # the bent stripe cannot be rebuilt: its flag alone, the call raises
    # the batch clean (every rebuilt cell of every tile compared), then with one byte bent in a late tile
    runs = [VerifyRun(dev, case, cell, seed=4100 + T + k, stripes=S, flips=flips)
            for flips in ([], C.late_flip(case, S, cell))]
    st = torch.cuda.Stream()
    before = jit_launches()
    for run in runs:
        run.run(st.cuda_stream)
    assert jit_launches() - before == len(runs)


@needs_measurement_build
@pytest.mark.parametrize("grid", C.BLOCK_GRIDS)
@pytest.mark.parametrize("k,m", C.BLOCK_ENCODE)
def test_block_tile_encode_loops(dev, k, m, grid):
    """The block-tile encode (the product's default instantiation, compiled by
    the measurement build as well) on a grid of 1 and 5 blocks (tune key 7): 12
    or 18 tiles, every block takes several."""
    xlib = H.experimental_lib()
    run = EncodeRun(dev, "rs", k, m, C.BLOCK_STRIPES, C.BLOCK_CELL, seed=5000 + 10 * k + m + grid, lib=xlib)
    try:
        H.tune_set(7, grid, xlib)
        on_side_stream(run, ("grid", grid))
    finally:
        H.tune_set(7, 0, xlib)


@needs_measurement_build
@pytest.mark.parametrize("grid", C.BLOCK_GRIDS)
@pytest.mark.parametrize("k,m,e", C.BLOCK_VERIFY)
def test_block_tile_generic_verify_loops(dev, k, m, e, grid):
    """The generic decode + verify kernel on a grid of 1 and 5 blocks.  Each
    (shape, grid) has a decode plan no other test uses, and a plan's first call
    only queues its compile: the launch counter must stay flat.  That holds
    once a process: a second run of this test in the same process (a rerun
    plugin) finds the plan compiled, takes the specialised kernel and fails the
    last assertion.  No tune holds the JIT off without also changing the
    kernel: it accepts every slab count, load schedule and queue setting, and
    another checksum scheme is another instantiation."""
    xlib = H.experimental_lib()
    case = C.VerifyCase(k, m, e, C.CRC32C, C.block_lost(k, e, grid), (), (C.BLOCK_CELL,),
                        "block-%d-%d-e%d-grid%d" % (k, m, e, grid))
    run = VerifyRun(dev, case, C.BLOCK_CELL, seed=5100 + 10 * k + grid, stripes=C.BLOCK_STRIPES, lib=xlib)
    before = jit_launches(xlib)
    try:
        H.tune_set(7, grid, xlib)
        run.run(torch.cuda.Stream().cuda_stream, ("grid", grid))
    finally:
        H.tune_set(7, 0, xlib)
    assert jit_launches(xlib) == before, "the specialised kernel ran in place of the generic one"


# ---- 3. one stream, both counter sets, and a graph ------------------------------------------

def sequence_runs(dev, k, m, graph):
    """[fused large, fused 1 tile, plain, fused 9 tiles] of sequence_tiles."""
    wave_tile = 8192 if k <= 6 else 4096
    runs = []
    for x, T in enumerate(C.sequence_tiles(cu_count(), graph)):
        S, cell = C.queue_shape(T, wave_tile)
        if x == 2:
            runs.append(PlainRun(dev, k, m, S, cell, seed=6000 + k))
        else:
            runs.append(EncodeRun(dev, "rs", k, m, S, cell, seed=6001 + 10 * x + k, tag="T %d" % T))
    return runs


@pytest.mark.parametrize("k,m", C.SEQUENCE_KM)
def test_fused_and_plain_launches_back_to_back(dev, k, m):
    """Eight launches queued on one stream with nothing between them: fused
    encode with 3 W + 5 tiles, with 1 tile, a plain hec_encode_device, fused
    with 9 tiles, and the same four again into buffers of their own.  The
    stream's two counter sets alternate, so the set a large launch leaves high
    is the set the launch after next needs zero; all checked after one
    synchronise."""
    first = sequence_runs(dev, k, m, graph=False)
    runs = first + [r.twin(dev) for r in first]
    for r in runs:
        r.clear()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    before = H.queue_stats(0)["streams"]
    for r in runs:
        r.launch(st.cuda_stream)
    st.synchronize()
    assert H.queue_stats(0)["streams"] - before <= 1
    for x, r in enumerate(runs):
        r.check(("launch", x))


@pytest.mark.parametrize("k,m", C.SEQUENCE_KM)
def test_fused_launches_in_one_graph(dev, k, m):
    """Four fused encode launches (2 CUs + 1 tiles, 1, 9 and 2 CUs + 1 again)
    captured as one chain: each takes a graph counter set of its own (4 per
    code, 8 of the process's 256 in all; see test_gpu_coding_launch.py
    ::test_tile_counts_in_one_graph for the budget).  Two replays, the outputs
    refilled with 0xA5 between them.  hec_decode_verify_device synchronises
    its stream and stays out of the capture."""
    large, one, _, nine = sequence_runs(dev, k, m, graph=True)
    runs = [large, one, nine, large.twin(dev)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for r in runs:  # once directly: every coder is warm before the capture
        r.clear()
        r.launch(side.cuda_stream)
    side.synchronize()
    for x, r in enumerate(runs):
        r.check(("direct", x))
    g0 = H.queue_stats(0)["graph_sets"]
    if g0 + len(runs) > 256:
        pytest.fail("the process has used up its graph counter sets before this test")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for r in runs:
            r.launch(torch.cuda.current_stream().cuda_stream)
    assert H.queue_stats(0)["graph_sets"] - g0 == len(runs)
    for rep in (1, 2):
        for r in runs:
            r.clear()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for x, r in enumerate(runs):
            r.check(("replay", rep, x))
    del g
