"""-m gpu: bench.py end to end on a small stack (8 keyframes), each run in a fresh process.  A plain run measures the headline
block alone, for exactly --steps timed steps, and --dump-outputs writes that block's last step; --full still carries every
other block of the line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8


def run_bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "BSLAM_BENCH_DRY_RUN", "BSLAM_BENCH_ONLY")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--keyframes", str(K)] + args, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_only_and_dumps_its_last_step(tmp_path):
    out = tmp_path / "outputs"
    line = run_bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert sum(line["config"]["gn_iteration_histogram"].values()) == 3 * K      # K keyframes in each of the 3 timed steps
    assert not {"roofline", "pcg", "cpu_baseline"} & set(line)
    assert not {"secondary", "trajectory", "survey", "strong", "in_bounds_pair_fraction"} & set(line["config"])
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sum(os.path.getsize(out / (k + ".npy")) for k in files) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    S = line["config"]["surfels_per_gpu"]
    assert files["poses"].shape == (K, 7) and np.isfinite(files["poses"]).all()
    assert np.abs(np.linalg.norm(files["poses"][:, :4], axis=1) - 1).max() < 1e-3
    assert files["gn_iterations"].shape == (K,) and files["gn_iterations"].sum() > 0
    assert len(files["surfel_index"]) == S and files["surfel_positions"].shape == (S, 3)
    assert np.isfinite(files["surfel_positions"]).all() and (files["surfel_active"] > 0).any()


def test_full_run_keeps_every_other_block():
    line = run_bench(["--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.2"])
    assert line["steps"] == 2 and line["value"] > 0
    assert line["roofline"]["kernel"] == "pose_accumulate_kernel" and line["roofline"]["launches"] > 0
    assert 0 < line["config"]["in_bounds_pair_fraction"] <= 1
    assert line["config"]["secondary"]["value"] > 0 and "roofline" in line["config"]["secondary"]
    assert line["pcg"]["headline_stack"]["value"] > 0 and line["pcg"]["secondary_stack"]["value"] > 0
    assert line["cpu_baseline"]["value"] > 0
