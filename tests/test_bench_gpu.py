"""``python bench.py`` as the driver runs it (one GPU, small batch, few steps).  With ``--full``: the step must come from
its launch plan, the tuner's in-step stage must run and leave a working table, and the line must carry the fields the
contract and DESIGN.md name.  Plain: the headline fields only, and ``--dump-outputs`` writes what the last timed step
computed, the same in every run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def test_default_line_replays_its_plan_and_refines_tiles_in_the_step():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "FS2_GEMM_TUNE")}
    env.update(FS2_REFINE_TOP="6", FS2_REFINE_CANDIDATES="2")
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--batch", "4", "--steps", "6", "--warmup", "2", "--full",
                        "--no-extra-legs", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 6 and line["value"] > 0 and line["scaling"] == "weak"
    assert line["dtype"] == "f32" and line["config"]["precision"] == "32-true" and line["vs_baseline"] is None
    plan = line["launch_plan"]
    assert plan["replayed_steps"] >= 6 and plan["launches_per_step"] > 300 and plan["segments"] == 1
    assert 0 < line["host_enqueue_ms_per_step"] < line["host_loop_ms_per_step"] + 50
    roof = line["roofline"]
    assert roof["bound"] == "mfma" and roof["peak"] == 157.3 and 0 < roof["frac"] < 1 and "time_source" in roof
    assert "in-step tile refinement:" in r.stderr
    assert line["loss_total"] == line["loss_total"]  # finite


def test_plain_run_writes_the_same_outputs_whatever_the_warm_up(tmp_path):
    """No ``--full``: exactly ``--steps`` timed steps, the secondary measurements null.  ``--dump-outputs`` writes the last
    timed step's loss terms, forward outputs, parameters and gradient as float32 .npy within 64 MB, and the timed steps
    start from the seeded initial state: runs with different warm-up lengths write the same arrays (tile tuner off, so
    that both sum in the same order)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(FS2_GEMM_TUNE="0")
    dumps = []
    for warmup in (1, 4):
        out = tmp_path / f"warmup{warmup}"
        r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--batch", "4", "--steps", "3", "--warmup", str(warmup),
                            "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == warmup and line["dtype"] == "f32" and line["higher_is_better"] is True
        assert line["launch_plan"]["replayed_steps"] >= 3
        frames = line["config"]["real_frames_per_step"]
        assert abs(line["value"] - frames / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"]
        for k in ("roofline", "cpu_baseline", "split_fp32", "bf16_mixed_b64", "learn_alignment", "gst_bf16_b64",
                  "host_enqueue_ms_per_step"):
            assert line[k] is None, k
        files = {p.name: np.load(p) for p in out.glob("*.npy")}
        assert {"loss_total.npy", "loss_spec.npy", "output.npy", "postnet_output.npy", "parameters.npy",
                "gradient.npy"} <= set(files), sorted(files)
        assert all(a.dtype == np.float32 for a in files.values())
        assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64 << 20
        assert abs(float(files["loss_total.npy"]) - line["loss_total"]) <= 1e-5 * max(1.0, abs(line["loss_total"]))
        dumps.append(files)
    a, b = dumps
    assert set(a) == set(b)
    for name in a:
        assert a[name].shape == b[name].shape, name
        scale = max(float(np.abs(a[name]).max()), 1e-30)
        assert float(np.abs(a[name] - b[name]).max()) <= 1e-5 * scale, name
