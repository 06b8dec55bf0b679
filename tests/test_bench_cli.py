"""bench.py's command line: a plain run does the timed steps only, `--full`
brings the other legs back, `--dump-outputs` writes what the last timed step
computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def test_full_is_off_by_default():
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs == ""
    a = bench.parse(["--full", "--dump-outputs", "d", "--steps", "3"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 3


def test_dump_outputs_sample_is_fixed_and_masked(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    rng = np.random.default_rng(1)
    small = torch.from_numpy(rng.integers(0, 256, (2, 3, 100), dtype=np.uint8))  # 600 <= 1000: whole
    big = torch.from_numpy(rng.integers(0, 256, (5, 4, 128), dtype=np.uint8))  # 2560 > 1000: sampled
    mask = torch.tensor([[True, False, False, True]] * 5)
    info = bench.dump_outputs(str(tmp_path / "a"), {"parity": (small, None), "rebuilt": (big, mask)}, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), {"parity": (small, None), "rebuilt": (big.clone(), mask)}, 0, 1)
    par = np.load(tmp_path / "a" / "parity.npy")
    reb = np.load(tmp_path / "a" / "rebuilt.npy")
    assert par.dtype == np.float32 and np.array_equal(par, small.numpy().reshape(-1).astype(np.float32))
    assert info["parity"]["sample"] == "whole" and info["rebuilt"]["elements"] == 1000
    assert reb.dtype == np.float32 and reb.shape == (1000,)
    assert np.array_equal(reb, np.load(tmp_path / "b" / "rebuilt.npy"))
    # every sampled value is a byte of the output at a cell the step wrote, or 0
    pos = np.sort(np.random.default_rng([bench.DUMP_SEED, 1, 5, 4, 128]).integers(0, big.numel(), size=1000))
    want = big.numpy().reshape(-1)[pos].astype(np.float32)
    want[~mask.numpy().reshape(-1)[pos // 128]] = 0
    assert np.array_equal(reb, want)
    # more than one rank: one file per rank
    bench.dump_outputs(str(tmp_path / "c"), {"parity": (small, None)}, 1, 2)
    assert os.listdir(tmp_path / "c") == ["parity_rank1.npy"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path, c_oracle):
    import ec_oracle
    k, m, S, cell = 6, 3, 5, 4096 + 64
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                          "1", "--spinup", "0", "--stripes", str(S), "--cell", str(cell), "--dump-outputs",
                          str(tmp_path / "o")], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u8"
    # value = data bytes of encode + decode per second, from the same elapsed time as ms_per_step
    assert d["value"] == pytest.approx(2 * k * cell * S / (d["ms_per_step"] * 1e-3) / bench.GIB, rel=1e-2, abs=0.006)
    # nothing beside the headline figure ran
    assert not {"host_path", "extra_configs", "cpu_baseline_parallel", "cpu_baseline_configs", "crc32c"} & set(d)
    assert d["cpu_baseline"] is None and d["parity_check"].startswith("not checked")
    assert sorted(os.listdir(tmp_path / "o")) == ["parity.npy", "rebuilt.npy"]
    par = np.load(tmp_path / "o" / "parity.npy")
    reb = np.load(tmp_path / "o" / "rebuilt.npy")
    assert par.dtype == np.float32 and par.shape == (S * m * cell,) and reb.shape == (S * m * cell,)
    # the inputs are the seeded batch the run states; its parity per the
    # oracle is what the dump holds, and the rebuilt cells are data 0..m-1
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0x5EED_EC00)
    data = torch.randint(0, 256, (S, k, cell), dtype=torch.uint8, device="cuda:0", generator=g).cpu().numpy()
    want = np.stack([np.stack(ec_oracle.c_encode(c_oracle, k, m, list(data[s]))) for s in range(S)])
    assert np.array_equal(par, want.reshape(-1).astype(np.float32))
    assert np.array_equal(reb, data[:, :m].reshape(-1).astype(np.float32))
