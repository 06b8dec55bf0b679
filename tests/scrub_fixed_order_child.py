"""Child process of test_gpu_scrub_variants.py::test_fixed_tile_order_in_child_process
(not collected by pytest).  Uses up the device's 256 graph counter sets with
captured launches that never run, then captures one graph G whose launches all
get an empty lease and so run their fixed-order kernels, replays G twice and
checks every output: scrub against _ref_batch, coding against the C oracle
and the original bytes, sentinels where nothing may be written.  Exit status 0
and a last line "fixed order ok" mean success."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hdfs-native_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ec_oracle as O  # noqa: E402
import hdfs_native_ec as H  # noqa: E402
from test_gpu_scrub import S, TILE, _ref_batch, consistent_stripes, stream  # noqa: E402
from test_gpu_scrub_variants import launch, loop_shape, spread_corruptions  # noqa: E402

SENTINEL = 0xA5
GRAPH_SETS = 256  # kGraphSets, csrc/ec_kernels.hip


def graph_sets():
    return H.queue_stats(0)["graph_sets"]


def main():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    dev = torch.device("cuda:0")
    c_oracle = O.load_c_oracle()
    coders = {}

    def coder(k, m, codec="rs"):
        if (k, m, codec) not in coders:
            coders[(k, m, codec)] = H.Coder(k, m, 0, codec=codec)
        return coders[(k, m, codec)]

    # ---- static buffers and the two data sets, all before any capture --------
    # scrub: (codec, k, m, stripes, cell); the last is the more-tiles-than-waves
    # shape, where a wave's tile + fx_step is still inside the batch
    big_s, big_cell = loop_shape(6)
    scrubs = [("xor", 2, 1, S, TILE[2] + 16), ("rs", 3, 2, S, TILE[3] + 16), ("rs", 6, 3, S, TILE[6] + 16),
              ("rs", 10, 4, S, TILE[10] + 16), ("xor", 6, 1, S, TILE[6] + 16)]
    # the other (k, m) the register kernel is built for: one wave-tile + a short chunk
    scrubs += [("rs", k, m, S, TILE[k] + 16) for k in (2, 3, 6, 10) for m in (1, 2, 3, 4)
               if (k, m) not in {(2, 1), (3, 2), (6, 3), (10, 4), (6, 1)}]
    scrubs += [("rs", 6, 3, big_s, big_cell)]
    s_img, s_want = [[], []], [[], []]  # per replay: numpy images, expected results
    for x, (codec, k, m, stripes, cell) in enumerate(scrubs):
        clean = consistent_stripes(codec, k, m, stripes, cell)
        for rep in range(2):
            cells = clean.copy()
            spread_corruptions(cells, k, m, seed=1000 + 100 * rep + x)
            s_img[rep].append(cells)
            s_want[rep].append(_ref_batch(codec, k, m, cells))
        assert not np.array_equal(s_want[0][x], s_want[1][x])
    s_buf = [torch.zeros(i.shape, dtype=torch.uint8, device=dev) for i in s_img[0]]
    s_res = [torch.full((i.shape[0], 2), -1, dtype=torch.int64, device=dev) for i in s_img[0]]
    # coding: encode and decode (first m data units lost) for (6,3) and (10,4)
    cs, ccell = 7, 3 * 65536 + 48
    codings = [(6, 3), (10, 4)]
    c_data = [[np.random.default_rng(40 + 10 * rep + k).integers(0, 256, size=(cs, k, ccell), dtype=np.uint8)
               for k, _ in codings] for rep in range(2)]
    c_d = [torch.zeros((cs, k, ccell), dtype=torch.uint8, device=dev) for k, _ in codings]
    c_p = [torch.zeros((cs, m, ccell), dtype=torch.uint8, device=dev) for _, m in codings]
    c_o = [torch.zeros((cs, k, ccell), dtype=torch.uint8, device=dev) for k, _ in codings]
    # reconstruct (6,3): data unit 2 and parity unit 7 lost, rebuilt into r_out
    lost = (2, 7)
    r_img = [consistent_stripes("rs", 6, 3, cs + rep, ccell)[:cs] for rep in range(2)]  # two different batches
    r_buf = torch.zeros((cs, 9, ccell), dtype=torch.uint8, device=dev)
    r_out = torch.zeros((cs, 9, ccell), dtype=torch.uint8, device=dev)

    def run_all():
        for (codec, k, m, _, _), buf, res in zip(scrubs, s_buf, s_res):
            launch(coder(k, m, codec), buf, res)
        for (k, m), d, p, o in zip(codings, c_d, c_p, c_o):
            H.encode_batch(coder(k, m), d, p)
            H.decode_batch(coder(k, m), d, p, list(range(m)), o)
        ptrs, strides = H.stripe_layout_ptrs(r_buf, 9)
        optrs, ostrides = H.stripe_layout_ptrs(r_out, 9)
        coder(6, 3).reconstruct_device([None if i in lost else p for i, p in enumerate(ptrs)], strides, optrs,
                                       ostrides, ccell, cs, stream=stream())

    # ---- use up the graph counter sets: captured, never launched --------------
    first = graph_sets()
    assert first == 0, first
    small = torch.from_numpy(consistent_stripes("rs", 6, 3, 1, 16)).to(dev)
    small_res = torch.zeros((1, 2), dtype=torch.int64, device=dev)
    run_all()  # once directly: every coder and plan exists before a capture begins
    torch.cuda.synchronize()
    assert graph_sets() == 0
    unused = []
    for _ in range(4):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_SETS // 4):
                launch(coder(6, 3), small, small_res)
        unused.append(g)
    before = graph_sets()
    assert before == GRAPH_SETS, before

    # ---- G: every launch below gets an empty lease ----------------------------
    G = torch.cuda.CUDAGraph()
    with torch.cuda.graph(G):
        run_all()
    after = graph_sets()
    assert after == GRAPH_SETS, after  # no launch of G took a counter set: all run the fixed order
    print(f"graph_sets {first} -> {before} -> {after}", flush=True)

    # ---- two replays with different data ---------------------------------------
    for rep in range(2):
        for buf, res, img in zip(s_buf, s_res, s_img[rep]):
            buf.copy_(torch.from_numpy(img))
            res.fill_(-1)
        for d, p, o, data in zip(c_d, c_p, c_o, c_data[rep]):
            d.copy_(torch.from_numpy(data))
            p.fill_(SENTINEL)
            o.fill_(SENTINEL)
        r_buf.copy_(torch.from_numpy(r_img[rep]))
        for u in lost:
            r_buf[:, u].fill_(0xEE)  # the lost units' slots are not read
        r_out.fill_(SENTINEL)
        torch.cuda.synchronize()
        G.replay()
        torch.cuda.synchronize()
        for x, (res, want) in enumerate(zip(s_res, s_want[rep])):
            got = res.cpu().numpy().view(np.uint64)
            assert np.array_equal(got, want), ("scrub", rep, scrubs[x],
                                               np.nonzero((got != want).any(axis=1))[0].tolist())
        for (k, m), d, p, o, data in zip(codings, c_d, c_p, c_o, c_data[rep]):
            O.c_check_batch(c_oracle, k, m, data, p.cpu().numpy(), threads=4)
            out = o.cpu().numpy()
            assert np.array_equal(out[:, :m], data[:, :m]), ("decode", rep, k, m)
            assert (out[:, m:] == SENTINEL).all(), ("decode wrote a present unit", rep, k, m)
            assert np.array_equal(d.cpu().numpy(), data), ("inputs changed", rep, k, m)
        out = r_out.cpu().numpy()
        for u in range(9):
            if u in lost:
                assert np.array_equal(out[:, u], r_img[rep][:, u]), ("reconstruct", rep, u)
            else:
                assert (out[:, u] == SENTINEL).all(), ("reconstruct wrote a present unit", rep, u)
    assert graph_sets() == GRAPH_SETS
    del G, unused
    for c in coders.values():
        c.close()
    print("fixed order ok", flush=True)


if __name__ == "__main__":
    main()
