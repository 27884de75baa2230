"""bench.py's command line: a plain run times the steps and nothing else (roofline and cpu_baseline
null), --full adds them, --dump-outputs DIR writes the last timed step's logits (fp32, seeded inputs:
equal bit for bit to an in-process forward of the same images), --steps sets the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_defaults_and_new_options():
    a = bench.parse([])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 20, 5, False, "")
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "d"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, True, "d")
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_fp32_and_seeded_sample(tmp_path, monkeypatch):
    t = torch.arange(100 * 16, dtype=torch.float64).reshape(100, 16)
    bench.dump_outputs(str(tmp_path / "a"), {"logits": t})
    a = np.load(tmp_path / "a" / "logits.npy")
    assert a.dtype == np.float32 and np.array_equal(a, t.numpy().astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)  # 64 rows of 16 fp32
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"logits": t})
    b, c = np.load(tmp_path / "b" / "logits.npy"), np.load(tmp_path / "c" / "logits.npy")
    assert b.dtype == np.float32 and b.shape == (64, 16) and b.nbytes <= 4096
    assert np.array_equal(b, c)                       # the same rows every run
    rows = (b[:, 0] / 16).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(b, a[rows])


def _run(extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--model", "deit_tiny",
           "--batch", "8", "--warmup", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_outputs(gpu, tmp_path):
    line = _run(["--steps", "3", "--dump-outputs", str(tmp_path / "out")])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0 and line["logits_finite"]
    # value and ms_per_step are the same measurement (both rounded on the line)
    assert abs(line["value"] * line["ms_per_step"] / 1e3 / 8 - 1) < 1e-2
    assert os.listdir(tmp_path / "out") == ["logits.npy"]
    got = np.load(tmp_path / "out" / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (8, 1000)
    # bench.py's images (seed 1000 on cuda) and weights (seed 0) through the model in this process
    from edgevisiontransformer_amd.modeling.models import vit
    g = torch.Generator(device="cuda").manual_seed(1000)
    img = torch.randn((8, 3, 224, 224), generator=g, device="cuda", dtype=torch.float32)
    ref = vit.build_named("deit_tiny", dtype="bf16", seed=0, max_batch=8)(img)
    torch.cuda.synchronize()
    assert np.array_equal(got, ref.float().cpu().numpy())


@pytest.mark.gpu
def test_full_run_adds_roofline_and_cpu_baseline(gpu):
    line = _run(["--steps", "2", "--full", "--cpu-seconds", "0.2"])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    roof, cpu = line["roofline"], line["cpu_baseline"]
    assert roof["role"] in roof["per_role"] and roof["avg_launch_us"] > 0 and roof["achieved"] > 0
    assert cpu["value"] > 0 and cpu["unit"] == "images/s"
