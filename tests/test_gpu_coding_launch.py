"""The plain coding launch (hec_gf_matmul_device, hec_encode_device,
hec_decode_device and the register kernel gf_matmul_v16 behind them) pinned
where its startup chain and tail keep being changed:

  1. every GF(2^8) product in every byte lane: matrices whose entries take
     every value 0..255 over inputs in which every 16-byte block position sees
     every byte, for each compile-time-k kernel (k = 2, 3, 6, 10; r = 1..4),
     the runtime-k kernel (k = 5, 12), the dword kernel with its byte tail and
     the byte kernel alone;
  2. tile counts on every branch of the work queue's deal, as direct launches
     back to back on one stream (large and tiny alternating, both counter
     sets) and once more captured into a graph;
  3. the kernels a launch without counters runs, in child processes
     (coding_fixed_order_child.py): past the 256 graph counter sets for every
     launch a graph can hold, past the 4096 stream sets for the verified read.

The reference is the oracle throughout (ec_oracle.matmul_shards, the C oracle's
encode and decode), never another device kernel.  Every buffer is compared as a
whole image (test_gpu_reconstruct_crc_rows.py): rows have a pitch of cell + 64,
outputs start as 0xA5 everywhere, input gaps and lost cells hold 0xEE, and
after a run every output buffer equals its expected image -- pitch gaps, rows
nobody asked for and a decode's present units still 0xA5 -- and every input
buffer is unchanged."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import coding_launch_cases as C
import ec_oracle as O
import hdfs_native_ec as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
SENT = 0xA5     # every output byte before a run
GARBAGE = 0xEE  # input pitch gaps and lost cells
BAND = 0xC3     # around a workspace


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


_coders = {}


def coder(k, m):
    if (k, m) not in _coders:
        _coders[(k, m)] = H.Coder(k, m, 0)
    return _coders[(k, m)]


_clib = []


def clib():
    if not _clib:
        _clib.append(O.load_c_oracle())
    return _clib[0]


class Rows:
    """A [stripes, units, pitch] device buffer and its host image.  For an
    input the image is what upload() puts there and check() proves unchanged;
    for an output clear() fills the device side and the image is what the run
    must leave.  base_off moves every base off the allocation's 16-byte grid."""

    def __init__(self, dev, stripes, units, cell, fill, pitch=None, base_off=0):
        self.S, self.units, self.cell, self.fill = stripes, units, cell, fill
        self.pitch = cell + C.PITCH_GAP if pitch is None else pitch
        n = stripes * units * self.pitch
        self.raw = torch.full((n + base_off,), fill, dtype=torch.uint8, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.view = self.raw[base_off:].view(stripes, units, self.pitch)
        self.image = np.full((stripes, units, self.pitch), fill, dtype=np.uint8)

    def ptrs(self, first_stripe=0):
        base = self.view.data_ptr() + first_stripe * self.units * self.pitch
        return [base + u * self.pitch for u in range(self.units)]

    def strides(self):
        return [self.units * self.pitch] * self.units

    def expect(self, cells, unit0=0):
        """cells [stripes, n, cell] into units unit0 .. unit0 + n - 1 of the image."""
        self.image[:, unit0:unit0 + cells.shape[1], :self.cell] = cells

    def reset(self):
        self.image[...] = self.fill

    def upload(self):
        self.view.copy_(torch.from_numpy(self.image))

    def clear(self):
        self.raw.fill_(self.fill)

    def check(self, what, free=()):
        """free = [(stripe, unit)]: cells whose [0, cell) is unspecified."""
        got, exp = self.view, torch.from_numpy(self.image).to(self.view.device)
        lead = self.raw[:self.raw.numel() - self.view.numel()]  # the base_off bytes in front of the first row
        assert bool((lead == self.fill).all()), (what, "bytes in front of the first row", lead.tolist())
        if free:
            got = got.clone()
            for s, u in free:
                got[s, u, :self.cell] = exp[s, u, :self.cell]
        if torch.equal(got, exp):
            return
        ne = got != exp
        pairs = ne.any(dim=2).nonzero().tolist()
        s, u = pairs[0]
        first = ne[s, u].nonzero()[0].item()
        raise AssertionError((what, "cells [stripe, unit] that differ", pairs[:16], "of", len(pairs), "first offset",
                              first, "got", int(got[s, u, first]), "want", int(exp[s, u, first]), "cell", self.cell))


def encode_ref(k, m, data):
    """The C oracle's parity of data [S, k, cell]: [S, m, cell]."""
    S, _, n = data.shape
    par = np.empty((S, m, n), dtype=np.uint8)
    d = np.ascontiguousarray(data)
    assert clib().orc_encode_batch(k, m, d.ctypes.data, n, S, par.ctypes.data) == 0
    return par


def decode_ref(k, m, data, parity, present):
    """The C oracle's decode of the batch with the units of `present`: the
    missing data units in ascending order, [S, e, cell]."""
    S, _, n = data.shape
    e = sum(1 for i in range(k) if not (present >> i) & 1)
    out = np.empty((S, e, n), dtype=np.uint8)
    d, p = np.ascontiguousarray(data), np.ascontiguousarray(parity)
    assert clib().orc_decode_batch(k, m, d.ctypes.data, p.ctypes.data, n, S, ctypes.c_uint64(present),
                                   out.ctypes.data) == 0
    return out


# ---- 1. every GF(2^8) product, in every byte lane ------------------------------------

class ProductRun:
    """Every matrix of product_matrices(k, r) over product_cells(k, route)
    through hec_gf_matmul_device, each into rows of its own of one output
    buffer.  route: "aligned" (the register kernels), "unaligned" (every base
    one byte off the 16-byte grid: the dword kernel and its byte tail),
    "unaligned-pitch" (the same with the plain pitch of cell + 64, so the bases
    take many misalignments) and "bytes" (7-byte cells: the byte kernel alone)."""

    def __init__(self, dev, k, r, route="aligned"):
        self.k, self.r, self.route = k, r, route
        self.cells_route = "unaligned" if route.startswith("unaligned") else route
        self.mats = C.product_matrices(k, r)
        cells = C.product_cells(k, self.cells_route)
        self.S, _, self.cell = cells.shape
        off = 1 if route.startswith("unaligned") else 0
        pitch = None
        if route == "unaligned":
            pitch = -(-(self.cell + C.PITCH_GAP) // 16) * 16
        self.inp = Rows(dev, self.S, k, self.cell, GARBAGE, pitch, off)
        self.out = Rows(dev, len(self.mats) * self.S, r, self.cell, SENT, pitch, off)
        if route == "unaligned":
            assert all(p % 16 == 1 for p in self.inp.ptrs() + self.out.ptrs(self.S))
        self.fill(0)

    def fill(self, rep):
        self.inp.expect(C.product_cells(self.k, self.cells_route, rep))
        self.inp.upload()
        want = C.product_expected(self.k, self.r, self.cells_route, rep)
        self.out.expect(want.reshape(len(self.mats) * self.S, self.r, self.cell))
        self.out.clear()

    def launch(self, stream):
        cod = coder(6, 3)  # the call takes its matrix and shapes from its arguments
        for t, mat in enumerate(self.mats):
            cod.gf_matmul_device(mat, self.inp.ptrs(), self.inp.strides(), self.out.ptrs(t * self.S),
                                 self.out.strides(), self.cell, self.S, stream)

    def check(self, what=""):
        # a differing output row (stripe, j) belongs to matrix stripe // S, row j
        self.out.check((what, "product", self.k, self.r, self.route, "stripes per matrix", self.S))
        self.inp.check((what, "product inputs", self.k, self.r, self.route))


def run_products(dev, k, r, route="aligned"):
    run = ProductRun(dev, k, r, route)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    run.launch(st.cuda_stream)
    st.synchronize()
    run.check()


@pytest.mark.parametrize("r", C.PRODUCT_R)
@pytest.mark.parametrize("k", C.PRODUCT_K)
def test_every_product_compile_time_k(dev, k, r):
    """gf_matmul_v16<K, R> on the work queue: every coefficient 0..255 (0
    included, which no RS matrix holds) times every byte in every lane."""
    run_products(dev, k, r)


@pytest.mark.parametrize("r", C.PRODUCT_R)
@pytest.mark.parametrize("k", C.RUNTIME_K)
def test_every_product_runtime_k(dev, k, r):
    """gf_matmul_v16<0, R>: 256-thread blocks at k = 5, 512-thread blocks at k = 12."""
    run_products(dev, k, r)


@pytest.mark.parametrize("route", ["unaligned", "unaligned-pitch", "bytes"])
def test_every_product_unaligned_and_byte_routes(dev, route):
    """k = 6, r = 3 off the 16-byte grid (gf_matmul_dw up to the last whole 8
    bytes, gf_matmul_bytes for the 5 behind them) and at 7-byte cells
    (gf_matmul_bytes alone)."""
    run_products(dev, 6, 3, route)


# ---- 2. small launches: tile counts around every branch of the queue ------------------

class CodeRun:
    """One (stripes, cell) batch of RS(k, m): hec_encode_device, hec_decode_device
    of the first m data units and, with mixed=True, hec_decode_device_mixed with
    mixed_masks and a workspace of exactly the advertised size between guard
    bands.  The decodes read the oracle's parity, not the encode's output."""

    def __init__(self, dev, k, m, stripes, cell, seed, mixed=False, tag=""):
        self.k, self.m, self.S, self.cell, self.seed, self.tag = k, m, stripes, cell, seed, tag
        self.cod = coder(k, m)
        n = k + m
        self.data = Rows(dev, stripes, k, cell, GARBAGE)
        self.par_in = Rows(dev, stripes, m, cell, GARBAGE)
        self.par_out = Rows(dev, stripes, m, cell, SENT)
        self.dec_out = Rows(dev, stripes, k, cell, SENT)
        self.lost = tuple(range(min(m, k)))
        self.mixed = mixed
        if mixed:
            self.masks = C.mixed_masks(k, m, stripes)
            self.mix_in = Rows(dev, stripes, n, cell, GARBAGE)
            self.mix_out = Rows(dev, stripes, k, cell, SENT)
            self.ws_bytes = self.cod.decode_mixed_workspace_size(stripes)
            self.ws_raw = torch.full((self.ws_bytes + 1024,), BAND, dtype=torch.uint8, device=dev)
            self.ws_off = 256 + (-self.ws_raw.data_ptr()) % 256
        self.fill(0)

    def fill(self, rep):
        k, m, S = self.k, self.m, self.S
        data = C.rs_data(k, S, self.cell, 7919 * self.seed + rep)
        par = encode_ref(k, m, data)
        self.data.expect(data)
        self.data.upload()
        self.par_in.expect(par)
        self.par_in.upload()
        self.par_out.expect(par)
        self.par_out.clear()
        present = ((1 << (k + m)) - 1) & ~sum(1 << i for i in self.lost)
        self.dec_out.reset()
        self.dec_out.expect(decode_ref(k, m, data, par, present), 0)
        self.dec_out.clear()
        if self.mixed:
            self.mix_in.reset()
            self.mix_in.expect(data, 0)
            self.mix_in.expect(par, k)
            self.mix_out.reset()
            for mask in set(self.masks):
                rows = [s for s in range(S) if self.masks[s] == mask]
                miss = [i for i in range(k) if not (mask >> i) & 1]
                rebuilt = decode_ref(k, m, data[rows], par[rows], mask)
                for x, i in enumerate(miss):
                    self.mix_out.image[rows, i, :self.cell] = rebuilt[:, x]
                for i in range(k + m):
                    if not (mask >> i) & 1:
                        self.mix_in.image[rows, i, :] = GARBAGE  # a lost cell is never read
            self.mix_in.upload()
            self.mix_out.clear()
            self.ws_raw.fill_(BAND)

    def encode(self, stream):
        self.cod.encode_device(self.data.ptrs(), self.data.strides(), self.par_out.ptrs(), self.par_out.strides(),
                               self.cell, self.S, stream)

    def decode(self, stream):
        shards = [None if i in self.lost else p for i, p in enumerate(self.data.ptrs())] + self.par_in.ptrs()
        self.cod.decode_device(shards, self.data.strides() + self.par_in.strides(), self.dec_out.ptrs(),
                               self.dec_out.strides(), self.cell, self.S, stream)

    def decode_mixed(self, stream):
        self.cod.decode_device_mixed(self.mix_in.ptrs(), self.mix_in.strides(), self.mix_out.ptrs(),
                                     self.mix_out.strides(), self.masks, self.cell, self.S,
                                     self.ws_raw.data_ptr() + self.ws_off, self.ws_bytes, stream)

    def launch(self, stream, flip=False, mixed=True):
        """encode then decode, or decode first with flip: over a sequence either
        call then counts on either counter set of the stream."""
        for call in ((self.decode, self.encode) if flip else (self.encode, self.decode)):
            call(stream)
        if self.mixed and mixed:
            self.decode_mixed(stream)
        return 2

    def check(self, what="", mixed=True):
        what = (what, "RS", self.k, self.m, "T", self.tag, "stripes", self.S, "cell", self.cell)
        self.par_out.check(what + ("parity",))
        self.dec_out.check(what + ("decode",))
        self.data.check(what + ("data changed",))
        self.par_in.check(what + ("parity input changed",))
        if self.mixed and mixed:
            self.mix_out.check(what + ("mixed decode",))
            self.mix_in.check(what + ("mixed decode inputs changed",))
            a, b = self.ws_off, self.ws_off + self.ws_bytes
            assert bool((self.ws_raw[:a] == BAND).all()) and bool((self.ws_raw[b:] == BAND).all()), what + ("band",)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("k", C.PRODUCT_K)
def test_tile_counts_back_to_back(dev, k):
    """T = 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, CUs - 1, CUs, CUs + 1 and
    2 CUs + 3 wave-tiles, as S x 1, 2, 3 or 5 tiles per stripe with a last tile
    of 16 bytes, W - 16 bytes or a full one: all launches queued on one stream
    with nothing between them, largest and smallest alternating, so a counter
    set left high by one launch is the set the launch after next needs zero."""
    m = C.RS[k]
    cases = C.tile_count_cases(k, cu_count())
    runs = [CodeRun(dev, k, m, S, cell, seed=100 * k + x, mixed=k in (6, 10), tag=name)
            for x, (_, S, cell, name) in enumerate(cases)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    before = H.queue_stats(0)["streams"]
    for x, run in enumerate(runs):
        run.launch(st.cuda_stream, flip=x % 2 == 1)
    st.synchronize()
    assert H.queue_stats(0)["streams"] - before <= 1
    for x, run in enumerate(runs):
        run.check(x)


@pytest.mark.parametrize("k", C.PRODUCT_K)
def test_tile_counts_in_one_graph(dev, k):
    """The encode and decode launches of T = 1, 7, 9 and CUs + 1 captured as
    one linear chain on one stream: every captured launch takes a graph counter
    set of its own, and two replays with different data are right.  (The mixed
    decode uploads its plans from the coder's pinned staging buffers, whose
    contents at replay time belong to later calls: it is not captured.)

    Budget: graph counter sets are never returned, and a process has 256 per
    device.  This test takes 10 per k, 40 in all, of the process that runs the
    suite; the other files' captures take about 30 together.  A test that adds
    captured queue launches has to keep the suite's total well below 256, or
    the files that run later (which do not all assert graph_sets) would
    silently take the fixed order."""
    m = C.RS[k]
    cases = [c for c in C.tile_count_cases(k, cu_count()) if c[3] in C.GRAPH_T]
    assert {c[3] for c in cases} == set(C.GRAPH_T) and len(cases) >= 5
    runs = [CodeRun(dev, k, m, S, cell, seed=300 * k + x, tag=name) for x, (_, S, cell, name) in enumerate(cases)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for x, run in enumerate(runs):  # once directly: every plan exists before the capture
        run.launch(side.cuda_stream, flip=x % 2 == 1)
    side.synchronize()
    for x, run in enumerate(runs):
        run.check(("direct", x))
    g0 = H.queue_stats(0)["graph_sets"]
    if g0 + 2 * len(runs) > 256:
        pytest.fail("the process has used up its graph counter sets before this test")
    g = torch.cuda.CUDAGraph()
    launches = 0
    with torch.cuda.graph(g, stream=side):
        for x, run in enumerate(runs):
            launches += run.launch(torch.cuda.current_stream().cuda_stream, flip=x % 2 == 1)
    assert H.queue_stats(0)["graph_sets"] - g0 == launches == 2 * len(runs)
    for rep in (1, 2):
        for run in runs:
            run.fill(rep)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for x, run in enumerate(runs):
            run.check(("replay", rep, x))
    del g


# ---- 3. the fixed-order fallbacks on the product build ---------------------------------

def test_fixed_order_fallbacks_in_child_process():
    """A launch that gets no counters runs another kernel: gf_matmul_v16<WQ =
    0> in place of the queue kernels, the generic fused kernels in place of the
    queue and plan-specialised ones.  That state is permanent for a process, so
    a child enters it (coding_fixed_order_child.py).  One child, started once."""
    child = subprocess.run([sys.executable, os.path.join(HERE, "coding_fixed_order_child.py")], capture_output=True,
                           text=True, timeout=600)
    assert child.returncode == 0, (child.returncode, child.stdout[-2000:], child.stderr[-4000:])
    assert "graph_sets 0 -> 256 -> 256" in child.stdout and "coding fixed order ok" in child.stdout, \
        child.stdout[-2000:]


def test_decode_verify_without_counters_in_child_processes():
    """hec_decode_verify_device waits for its flags, so no graph can hold it:
    its launch without counters is the one past 4096 streams with counter sets.
    RS(6,3) and RS(10,4) with the first m data units lost, both checksum types,
    clean and with one flipped survivor byte; the plan-specialised kernel must
    run before and the generic one after (hec_jit_stats).  Four children at
    once, one per code and type: each compiles one kernel."""
    jobs = [(k, ctype) for k in (6, 10) for ctype in (H.CHECKSUM_CRC32C, H.CHECKSUM_CRC32)]
    script = os.path.join(HERE, "coding_fixed_order_child.py")
    children = [subprocess.Popen([sys.executable, script, "verify", str(k), str(ctype)], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, text=True) for k, ctype in jobs]
    results = []
    try:
        for child in children:
            results.append(child.communicate(timeout=120))
    finally:
        for child in children:
            if child.poll() is None:
                child.kill()
                child.communicate()
    for (k, ctype), child, (out, err) in zip(jobs, children, results):
        assert child.returncode == 0, (k, ctype, child.returncode, out[-2000:], err[-4000:])
        assert "stream sets" in out and "-> 4096" in out and "decode + verify without counters ok" in out, \
            (k, ctype, out[-2000:])
