"""GPU: the launcher's mesh DSM (eonerf_code_amd/train_dp.py --mesh_out PATH together with --gt_dsm FILE): after the mesh is saved rank 0
rasterises it from above on the lidar DSM's grid and prints mesh/mae= once, with a finite value; without --gt_dsm the output has no such
key and the PLY holds the same bytes.  The scene and the step count are those of tests/test_train_dp_mesh_gpu.py."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 17


def run(logs, extra):
    # 2048 rays / 512 per step = 4 steps per epoch; step 16 is the last step
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "512", "--n_images", "2",
           "--n_samples", "64", "--max_train_steps", "16", "--check_every", "8", "--logs_dir", str(logs), "--exp_name", "t"] + extra
    # fixed-order gradient sums: two runs then hold the same weights bit for bit
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), EONERF_DETERMINISTIC="1")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_launcher_prints_the_mesh_mae_once_and_leaves_the_ply_alone(tmp_path):
    H = 32
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    gt = 30 + 6 * torch.sin(xx / 5) * torch.cos(yy / 7)
    gt_path = os.path.join(str(tmp_path), "gt.pt")
    torch.save({"dsm": gt, "roi": [1000.0, 5000.0, float(H), 0.5], "scene_offset": [1008.0, 5008.0, 30.0], "scene_scale": [8.0, 8.0, 40.0],
                "sun": [35.0, 160.0]}, gt_path)
    ply_a, ply_b = str(tmp_path / "a" / "scene.ply"), str(tmp_path / "b" / "scene.ply")
    # a level inside the density range of a field sixteen steps old, as in tests/test_train_dp_mesh_gpu.py
    mesh_flags = ["--mesh_res", str(RES), "--mesh_level", "0.3"]
    out = run(tmp_path / "with", ["--mesh_out", ply_a, "--gt_dsm", gt_path] + mesh_flags)
    found = re.findall(r"mesh/mae=(\S+) \| mesh/cells=(\d+)", out)
    assert len(found) == 1, out
    print("mesh/mae=" + found[0][0], "mesh/cells=" + found[0][1])
    assert math.isfinite(float(found[0][0])) and int(found[0][1]) > 0
    assert out.index("mesh=") < out.index("mesh/mae=") and "val/mae=" in out
    without = run(tmp_path / "without", ["--mesh_out", ply_b] + mesh_flags)
    assert "mesh/mae" not in without and "mesh=" in without
    assert os.path.getsize(ply_a) > 1000 and open(ply_a, "rb").read() == open(ply_b, "rb").read()
