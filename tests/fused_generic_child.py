"""Child process of test_gpu_fused_launch.py (not collected by pytest), started
once with HEC_JIT=0: in such a process no decode plan is ever specialised, so
every hec_decode_verify_device call below runs the ahead-of-time generic kernel
gf_fused_crc<K, E, SLABS, 12, KIND, true, 2, SLABS == 4> of its shape.

Runs every case of fused_launch_cases.generic_cases() at both cells through
VerifyRun (whole images against the oracle) and prints one JSON verdict a case:
{"case": name, "ok": true} or {"case": name, "ok": false, "error": ...}.  A
failed comparison goes on to the next case; any other error (a device error
among them) ends the child there, so nothing more is started on the GPU.

Then the launch without counters, the way coding_fixed_order_child.py reaches
it: the device's 256 graph counter sets are used up by captured launches that
never run, and one fused RS(3,2) encode + CRC of 36368-byte cells captured
after that gets an empty lease, runs the block-tile kernel in place of the
work-queue one and must leave the same images, over two replays.

Last line {"done": true, "cases": 26, "jit_launches": 0, "fixed_order": true};
exit status 0 only if every verdict is ok.  The child ends itself after LIMIT
seconds."""
import json
import os
import signal
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "hdfs-native_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import fused_launch_cases as C  # noqa: E402
import hdfs_native_ec as H  # noqa: E402
from test_gpu_fused_launch import EncodeRun, PlainRun, VerifyRun, _coders  # noqa: E402

LIMIT = 240
GRAPH_SETS = 256  # kGraphSets, csrc/ec_kernels.hip


def say(**verdict):
    print(json.dumps(verdict), flush=True)


def fixed_order_encode(dev):
    """One fused RS(3,2) encode + CRC past the graph counter sets."""
    side = torch.cuda.Stream()
    run = EncodeRun(dev, "rs", 3, 2, C.STRIPES, C.CELLS[1], seed=77)
    small = PlainRun(dev, 6, 3, 1, 16, seed=1)
    torch.cuda.synchronize()
    run.clear()
    run.launch(side.cuda_stream)  # once directly: the coder is warm before a capture
    small.launch(side.cuda_stream)
    side.synchronize()
    run.check("direct")
    assert H.queue_stats(0)["graph_sets"] == 0
    unused = []
    for _ in range(4):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(GRAPH_SETS // 4):
                small.launch(torch.cuda.current_stream().cuda_stream)
        unused.append(g)
    assert H.queue_stats(0)["graph_sets"] == GRAPH_SETS
    G = torch.cuda.CUDAGraph()
    with torch.cuda.graph(G, stream=side):
        run.launch(torch.cuda.current_stream().cuda_stream)
    assert H.queue_stats(0)["graph_sets"] == GRAPH_SETS  # an empty lease: block tiles in a fixed order
    for rep in (1, 2):
        run.clear()
        torch.cuda.synchronize()
        G.replay()
        torch.cuda.synchronize()
        run.check(("replay without counters", rep))
    del G, unused


def main():
    assert os.environ.get("HEC_JIT") == "0", "start with HEC_JIT=0"
    signal.alarm(LIMIT)
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream()
    cases, failed = C.generic_cases(), 0
    for x, case in enumerate(cases):
        try:
            for y, cell in enumerate(case.cells):
                VerifyRun(dev, case, cell, seed=9000 + 2 * x + y).run(st.cuda_stream)
            say(case=case.name, ok=True)
        except AssertionError as err:
            failed += 1
            say(case=case.name, ok=False, error=repr(err)[:1500])
        except Exception as err:  # the device may be in any state: stop here
            say(case=case.name, ok=False, error=repr(err)[:1500])
            return 2
    fixed = False
    try:
        fixed_order_encode(dev)
        fixed = True
    except AssertionError as err:
        say(fixed_order_error=repr(err)[:1500])
    launches = H.jit_stats()["launches"]
    for c in _coders.values():
        c.close()
    say(done=True, cases=len(cases), jit_launches=launches, fixed_order=fixed)
    return 0 if not failed and fixed and launches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
