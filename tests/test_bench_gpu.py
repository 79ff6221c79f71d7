"""-m gpu: the bench contract on a reduced workload -- one JSON line with the agreed keys (the driver parses exactly this)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    r = subprocess.run([sys.executable, "bench.py", "--gaussians", "200000", "--steps", "3", "--warmup", "1", "--vq-steps", "2",
                        "--full", "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["value"] > 0
    assert d["vs_baseline"] is None and "workload" in d["config"] and d["data"].startswith("synthetic")
    rf = d["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(rf) and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert d["device_allocs_in_timed_region"] == 0 and d["ranks_seen"] == 1
    assert set(d["roofline_blend"]) == {"render_forward", "render_backward"}
    assert all(0 < v["frac"] < 1 for v in d["roofline_blend"].values())
    vq = d["vq"]
    assert vq["value"] > 0 and vq["steps"] == 2 and vq["final_assignment_ms"] > 0 and vq["accumulate_first_step_ms"] > 0
    assert "error" not in json.dumps(d.get("qat_loop", {})) and "error" not in json.dumps(d.get("qat_model", {}))
    assert "error" not in json.dumps(d.get("vq", {})) and "error" not in json.dumps(d.get("postvq_index_layout", {}))


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline keys only, and --dump-outputs writes the last timed step's outputs (float32, <= 64 MiB)."""
    r = subprocess.run([sys.executable, "bench.py", "--gaussians", "200000", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["unit"] == "views/s"
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    assert d["device_allocs_in_timed_region"] == 0
    for k in ("roofline", "roofline_blend", "stages_ms", "qat_loop", "postvq_index_layout", "sizes", "heavy_tail", "qat_model",
              "vq", "cpu_baseline", "parity"):
        assert k not in d, k
    a = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert sum(f.stat().st_size for f in tmp_path.glob("*.npy")) <= 64 * 2 ** 20
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    n = 2 ** 17                                               # 200000 Gaussians: a sample of 2^17 rows
    shs, gs = 4096 + 20000, 4096 + 50000                      # codebooks of tests/synth.py index_scene: whole
    assert a["color"].shape == (3, 1080, 1920) and a["radii"].shape == (n,) and a["visible"].shape == (n,)
    for k, shape in (("means2D", (n, 3)), ("means3D", (n, 3)), ("opacities", (n, 1)), ("scale_factors", (n, 1)),
                     ("shs", (shs, 16, 3)), ("scales", (gs, 3)), ("rotations", (gs, 4))):
        assert a["grad_" + k].shape == shape, k
    assert a["color"].any() and (a["radii"] > 0).any() and a["grad_means3D"].any() and a["grad_shs"].any()
