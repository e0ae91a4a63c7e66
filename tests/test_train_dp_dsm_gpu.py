"""GPU: the launcher's on-device DSM validation (eonerf_code_amd/train_dp.py --gt_dsm): after every epoch rank 0 renders the nadir
DSM, registers it on the ground truth and prints val/mae on a status line; without the flag the launcher prints none."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(tmp_path, extra):
    # 8192 rays / 1024 per step = 8 steps per epoch; 17 steps = epochs 0 and 1 complete, one step of epoch 2
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "8192", "--batch_size", "1024", "--n_images", "5",
           "--max_train_steps", "17", "--logs_dir", str(tmp_path), "--exp_name", "t"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_launcher_prints_the_dsm_mae_after_every_epoch(tmp_path):
    H = 32
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    gt = 30 + 6 * torch.sin(xx / 5) * torch.cos(yy / 7)
    water = torch.zeros(H, H, dtype=torch.uint8)
    water[:4, :4] = 1
    path = os.path.join(str(tmp_path), "gt.pt")
    torch.save({"dsm": gt, "roi": [1000.0, 5000.0, float(H), 0.5], "water": water, "scene_offset": [1008.0, 5008.0, 30.0],
                "scene_scale": [8.0, 8.0, 40.0], "sun": [35.0, 160.0]}, path)
    out = run(tmp_path, ["--gt_dsm", path])
    vals = [float(m) for m in re.findall(r"val/mae=([^\s|]+)", out)]
    assert len(vals) == 2 and all(math.isfinite(v) and v >= 0 for v in vals), out
    assert re.search(r"epoch=1 \| .* \| step=16 \| val/mae=", out), out
    assert "step=0" in out and "rays/s=" in out


def test_launcher_without_the_flag_prints_no_validation_line(tmp_path):
    assert "val/" not in run(tmp_path, [])
