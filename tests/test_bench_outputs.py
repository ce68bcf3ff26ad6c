"""bench.py's run modes: a plain run times exactly --steps steps and prints the headline line only; --full adds the per-kernel rows;
--dump-outputs writes what the last timed step computed, the same files from run to run.

CPU part: dump_outputs itself on a stand-in engine (file names, float32, the size bound, seeded samples).  GPU part: the plain and
--full lines of a small configuration, and two plain runs whose dumped outputs must be bit-identical (the step is: see
test_gpu_benchcfg.py::test_deepfm_three_steps_are_bit_reproducible)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--batch", "4096", "--vocab", "20000"]


def _bench(args, timeout=400):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


_STANDIN = r"""
import sys, types, torch
sys.path.insert(0, sys.argv[1])
import bench
g = torch.Generator().manual_seed(0)
R, D, B, F = 50000, 16, 256, 4
eng = types.SimpleNamespace(loss=torch.tensor([0.5]), prob=torch.rand(B, generator=g), flat_params=torch.rand(3 << 20, generator=g),
                            table=torch.rand((R, D), generator=g), lin_w=torch.rand(R, generator=g),
                            ids=torch.randint(0, R // F, (B, F), generator=g), row_base=torch.arange(F) * (R // F))
bench.dump_outputs(eng, sys.argv[2], [("table", eng.table, eng.lin_w, eng.ids + eng.row_base)])
"""


def test_dump_outputs_writes_seeded_float32_samples(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        subprocess.run([sys.executable, "-c", _STANDIN, ROOT, d], check=True, timeout=120)
    a, b = _load(dirs[0]), _load(dirs[1])
    assert sorted(a) == ["dense_params", "loss", "prob", "table_lin_rows", "table_rows"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].tolist() == [0.5] and a["prob"].shape == (256,)
    assert a["dense_params"].shape == (1 << 20,)                     # 3 M elements: a sample, not the whole buffer
    n = 256 * 4 + 16384                                            # every row the batch touched (fewer than 16384), 16384 sampled rows
    assert a["table_rows"].shape == (n, 16) and a["table_lin_rows"].shape == (n,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0])) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_the_steps_asked_and_dumps_reproducible_outputs(tmp_path):
    dumps = []
    for r in range(2):
        d = str(tmp_path / ("run%d" % r))
        line = _bench(SMALL + ["--steps", "7", "--warmup", "3", "--dump-outputs", d])
        assert line["steps"] == 7 and line["warmup"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
        assert abs(line["value"] - 4096 * 1e3 / line["ms_per_step"]) <= 2e-3 * line["value"]
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["unit"] == "examples/sec"
        for key in ("roofline", "roofline_all", "cpu_baseline", "strict_fp32"):
            assert key not in line, key
        dumps.append(_load(d))
        assert abs(float(dumps[-1]["loss"][0]) - line["config"]["final_loss"]) <= 1e-6
    assert sorted(dumps[0]) == ["dense_params", "loss", "prob", "table_lin_rows", "table_rows"]
    for k in dumps[0]:
        assert dumps[0][k].dtype == np.float32
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_full_run_reports_the_kernel_rows():
    line = _bench(SMALL + ["--steps", "8", "--warmup", "2", "--full", "--events", "on", "--no-cpu-baseline"])
    assert line["steps"] == 8 and line["ms_per_step"] > 0
    assert line["config"]["per_kernel_events"] is True and line["roofline_all"] and line["roofline"] is not None
