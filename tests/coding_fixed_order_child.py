"""Child process of test_gpu_coding_launch.py::test_fixed_order_fallbacks_in_child_process
(not collected by pytest), after scrub_fixed_order_child.py: runs everything once
directly, uses up the device's 256 graph counter sets with captured launches
that never run, then captures one graph G whose launches all get an empty lease
and so run their fixed-order kernels, replays G twice with different data and
compares every buffer as a whole image with the oracle's.

G holds hec_gf_matmul_device with every matrix of part 1 for all 16 (k, r);
encode and decode of RS(2,1) and RS(3,2) at 3 * 16384 + 48-byte cells and 7
stripes (the fixed order's block tile is 16 KiB: full tiles, a partial last one
and the tile-order group's remainder); part 2's shapes of 1 and 9 wave-tiles at
every k; and hec_encode_crc_device for RS(3,2), RS(6,3) and RS(10,4) at
8208-byte cells with every stripe's sums from the oracle.

Exit status 0 and a last line "coding fixed order ok" mean success.

hec_decode_verify_device reads its flags back and waits for the stream, so it
cannot be captured.  Its launch without counters is reached the other way the
lease runs out, past 4096 streams with counter sets of their own, by
test_decode_verify_without_counters_in_child_processes: started as `verify K
TYPE`, the child compiles the plan-specialised kernel of RS(K, m) with the
first m data units lost (one compile is most of a child's time, so each code
and checksum type has a child of its own), gives 4096 streams one tiny launch
each, then runs the verified read on a further stream, clean and with one
flipped survivor byte (exactly that flag).  hec_jit_stats' launch count moves
with every call before and must not move after, which proves the generic
kernel ran in place of the plan-specialised one.  Last line "decode + verify
without counters ok"."""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hdfs-native_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import coding_launch_cases as C  # noqa: E402
import hdfs_native_ec as H  # noqa: E402
from test_gpu_coding_launch import (GARBAGE, SENT, CodeRun, ProductRun, Rows, _coders, clib, coder,  # noqa: E402
                                    cu_count, encode_ref)
from test_gpu_parity import _hip_runtime  # noqa: E402

GRAPH_SETS = 256    # kGraphSets, csrc/ec_kernels.hip
STREAM_SETS = 4096  # kMaxStreamSets, csrc/ec_kernels.hip
BPC = 512
CRC_CELL = 8208     # 16 chunks of 512 bytes and a short one; less than a block tile of the fused kernels


def graph_sets():
    return H.queue_stats(0)["graph_sets"]


def chunk_sums(cells, ctype):
    """The C oracle's chunk sums of cells [S, n, cell]: [S, n, nck, 4]."""
    S, n, cell = cells.shape
    nck = -(-cell // BPC)
    out = np.empty((S, n, nck, 4), dtype=np.uint8)
    cells = np.ascontiguousarray(cells)
    for s in range(S):
        for u in range(n):
            clib().orc_chunk_checksum(ctype, cells[s, u].ctypes.data, cell, BPC, out[s, u].ctypes.data)
    return out


class EncodeCrcRun:
    """hec_encode_crc_device: parity rows and the dense sums array, both
    sentinel-filled, against the oracle's parity and every chunk sum."""

    def __init__(self, dev, k, m, stripes, cell, seed):
        self.k, self.m, self.S, self.cell, self.seed = k, m, stripes, cell, seed
        self.data = Rows(dev, stripes, k, cell, GARBAGE)
        self.par = Rows(dev, stripes, m, cell, SENT)
        self.sums = torch.full((stripes, k + m, -(-cell // BPC), 4), SENT, dtype=torch.uint8, device=dev)
        self.fill(0)

    def fill(self, rep):
        data = C.rs_data(self.k, self.S, self.cell, 104729 * self.seed + rep)
        par = encode_ref(self.k, self.m, data)
        self.data.expect(data)
        self.data.upload()
        self.par.expect(par)
        self.par.clear()
        self.want = torch.from_numpy(chunk_sums(np.concatenate([data, par], axis=1), H.CHECKSUM_CRC32C))
        self.sums.fill_(SENT)

    def launch(self, stream):
        coder(self.k, self.m).encode_crc_device(self.data.ptrs(), self.data.strides(), self.par.ptrs(),
                                                self.par.strides(), self.cell, self.S, BPC, self.sums.data_ptr(), stream)

    def check(self, what=""):
        what = (what, "encode + CRC", self.k, self.m)
        self.par.check(what + ("parity",))
        self.data.check(what + ("data changed",))
        got = self.sums.cpu()
        assert torch.equal(got, self.want), what + ("sums [stripe, unit, chunk]",
                                                    (got != self.want).any(dim=3).nonzero()[:12].tolist())


class DecodeVerifyRun:
    """hec_decode_verify_device with the first m data units lost.  flip =
    (stripe, unit, byte) of one survivor cell, or None: every survivor is needed
    (k of k + m - m), so that stripe cannot be rebuilt -- ErasureCodingError,
    its flag set and no other, the other stripes rebuilt."""

    def __init__(self, dev, k, m, stripes, cell, ctype, flip, seed):
        self.k, self.m, self.S, self.cell, self.ctype, self.flip = k, m, stripes, cell, ctype, flip
        data = C.rs_data(k, stripes, cell, seed)
        par = encode_ref(k, m, data)
        self.lost = tuple(range(m))
        self.inp = Rows(dev, stripes, k + m, cell, GARBAGE)
        self.inp.expect(data, 0)
        self.inp.expect(par, k)
        self.inp.image[:, :m] = GARBAGE  # the lost units' slots are not read
        if flip:
            self.inp.image[flip] ^= 0x40
        self.inp.upload()
        self.out = Rows(dev, stripes, k, cell, SENT)
        self.out.expect(data[:, :m], 0)
        self.sums = torch.from_numpy(chunk_sums(np.concatenate([data, par], axis=1), ctype)).to(dev)
        self.bad = torch.full((stripes, k + m), 7, dtype=torch.uint8, device=dev)
        self.want_bad = np.zeros((stripes, k + m), dtype=np.uint8)
        if flip:
            self.want_bad[flip[0], flip[1]] = 1

    def run(self, stream):
        self.out.clear()
        self.bad.fill_(7)
        torch.cuda.synchronize()
        ptrs = [None if i in self.lost else p for i, p in enumerate(self.inp.ptrs())]
        try:
            coder(self.k, self.m).decode_verify_device(self.ctype, ptrs, self.inp.strides(), self.out.ptrs(),
                                                       self.out.strides(), self.cell, self.S, BPC,
                                                       self.sums.data_ptr(), self.bad.data_ptr(), stream)
            raised = False
        except H.ErasureCodingError:
            raised = True
        torch.cuda.synchronize()
        what = ("decode + verify", self.k, self.m, self.ctype, self.flip)
        assert raised == bool(self.flip), what
        got = self.bad.cpu().numpy()
        assert np.array_equal(got, self.want_bad), what + (np.argwhere(got != self.want_bad).tolist(),)
        free = [(self.flip[0], u) for u in self.lost] if self.flip else ()
        self.out.check(what, free=free)
        self.inp.check(what + ("inputs changed",))


class Clock:
    def __init__(self):
        self.t0 = time.perf_counter()

    def stamp(self, phase):
        print(f"{phase}: {time.perf_counter() - self.t0:.2f} s since start", flush=True)


def graph_main():
    """The fixed-order kernels of every capturable launch, through graph G."""
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    dev = torch.device("cuda:0")
    clock = Clock()
    side = torch.cuda.Stream()

    # ---- static buffers, all before any capture ---------------------------------------
    runs = [ProductRun(dev, k, r) for k in C.PRODUCT_K for r in C.PRODUCT_R]
    runs += [CodeRun(dev, k, m, 7, 3 * 16384 + 48, seed=900 + k, tag="block tiles") for k, m in ((2, 1), (3, 2))]
    x = 0
    for k in C.PRODUCT_K:
        for T, S, cell, name in C.tile_count_cases(k, cu_count()):
            if T in C.FIXED_ORDER_T:
                runs.append(CodeRun(dev, k, C.RS[k], S, cell, seed=950 + x, tag=name))
                x += 1
    assert x >= 3 * len(C.PRODUCT_K)
    runs += [EncodeCrcRun(dev, k, m, 5, CRC_CELL, seed=k) for k, m in ((3, 2), (6, 3), (10, 4))]
    clock.stamp("buffers")

    def run_all(stream):
        for run in runs:
            run.launch(stream)

    def check_all(what):
        for run in runs:
            run.check(what)

    # ---- once directly: every coder and plan exists before a capture begins ------------
    first = graph_sets()
    assert first == 0, first
    torch.cuda.synchronize()
    run_all(side.cuda_stream)
    side.synchronize()
    check_all("direct")
    assert graph_sets() == 0

    # ---- use up the graph counter sets: captured, never launched -----------------------
    small = CodeRun(dev, 6, 3, 1, 16, seed=1)
    torch.cuda.synchronize()
    unused = []
    for _ in range(4):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(GRAPH_SETS // 4):
                small.encode(torch.cuda.current_stream().cuda_stream)
        unused.append(g)
    before = graph_sets()
    assert before == GRAPH_SETS, before

    # ---- G: every launch below gets an empty lease -------------------------------------
    G = torch.cuda.CUDAGraph()
    with torch.cuda.graph(G, stream=side):
        run_all(torch.cuda.current_stream().cuda_stream)
    after = graph_sets()
    assert after == GRAPH_SETS, after  # no launch of G took a counter set: all run the fixed order
    print(f"graph_sets {first} -> {before} -> {after}", flush=True)

    # ---- two replays with different data ------------------------------------------------
    for rep in (1, 2):
        for run in runs:
            run.fill(rep % 2 if isinstance(run, ProductRun) else rep)
        torch.cuda.synchronize()
        G.replay()
        torch.cuda.synchronize()
        check_all(("replay", rep))
    assert graph_sets() == GRAPH_SETS
    del G, unused
    for c in _coders.values():
        c.close()
    clock.stamp("graph")
    print("coding fixed order ok", flush=True)


def verify_main(k, ctype):
    """hec_decode_verify_device of RS(k, m) and one checksum type past 4096 streams."""
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    dev = torch.device("cuda:0")
    clock = Clock()
    m = C.RS[k]
    side = torch.cuda.Stream()
    assert coder(k, m).prepare_decode(list(range(m)), ctype), "hiprtc unavailable on the GPU box"
    clock.stamp("JIT kernel")
    # clean, and the first survivor's last byte (in a short chunk) flipped
    verified = [DecodeVerifyRun(dev, k, m, 3, CRC_CELL, ctype, flip, seed=1000 + 10 * k + ctype)
                for flip in (None, (1, m, CRC_CELL - 1))]
    jit0 = H.jit_stats()["launches"]
    for v in verified:
        v.run(side.cuda_stream)
    assert H.jit_stats()["launches"] - jit0 == len(verified)  # with counters: the plan-specialised kernel, every time

    hip = _hip_runtime()
    small = CodeRun(dev, k, m, 1, 16, seed=1)
    torch.cuda.synchronize()
    streams0 = H.queue_stats(0)["streams"]
    handles = []
    while H.queue_stats(0)["streams"] < STREAM_SETS and len(handles) < STREAM_SETS:
        s = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # hipStreamNonBlocking
        handles.append(s)
        small.encode(s.value)  # the stream's first lease: its two sets
    torch.cuda.synchronize()
    streams1 = H.queue_stats(0)["streams"]
    assert streams1 == STREAM_SETS, (streams0, streams1, len(handles))
    clock.stamp("streams")
    last = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(last), 1) == 0
    jit1 = H.jit_stats()["launches"]
    for v in verified:
        v.run(last.value)
    assert H.jit_stats()["launches"] == jit1, "a plan-specialised kernel ran without counters"
    small.fill(1)
    torch.cuda.synchronize()
    small.launch(last.value)  # the plain launches there: the fixed order as well
    torch.cuda.synchronize()
    small.check("past the stream sets")
    assert H.queue_stats(0)["streams"] == STREAM_SETS
    print(f"stream sets {streams0} -> {streams1}, jit launches {jit0} -> {jit1} -> {H.jit_stats()['launches']}",
          flush=True)
    # the 4097 streams end with the process: destroying them one by one took 2.5 s
    for c in _coders.values():
        c.close()
    clock.stamp("teardown")
    print("decode + verify without counters ok", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "verify":
        verify_main(int(sys.argv[2]), int(sys.argv[3]))
    else:
        graph_main()
