"""GPU: the launcher with camera offset refinement (eonerf_code_amd/train_dp.py --rpc_correction): a few dozen steps on the synthetic
rays run clean, the status line carries pose/max_offset=, the checkpoint carries the offsets' key, and a run resumed from it starts with
the same table."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMG = 5


def launch(tmp_path, extra):
    # 2048 rays / 256 per step = 8 steps per epoch; checkpoints every 4 epochs: step 32 writes ckpts/epoch=4.ckpt
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "256", "--n_images", str(N_IMG),
           "--logs_dir", str(tmp_path), "--exp_name", "t", "--check_every", "8"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_launcher_learns_saves_and_resumes_the_offsets(tmp_path):
    out = launch(tmp_path, ["--rpc_correction", "--rpc_lr", "1e-4", "--max_train_steps", "33"])
    vals = [float(v) for v in re.findall(r"step=\d+ \| loss=\S+ \| rays/s=\d+ \| pose/max_offset=(\S+)\n", out)]
    assert len(vals) == 5 and vals[0] > 0 and all(0 < v < 1e-2 for v in vals), out      # steps 0, 8, .. 32; at most lr per step and component
    path = os.path.join(str(tmp_path), "t", "ckpts", "epoch=4.ckpt")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    po = ckpt["origin_offsets_state_dict"]
    assert tuple(po["origin_offsets"].shape) == (N_IMG, 3) and po["optimizer"] is not None
    want = po["origin_offsets"].norm(dim=1).max().item()
    assert want > 0
    out2 = launch(tmp_path, ["--rpc_correction", "--resume", path, "--max_train_steps", "0"])
    m = re.search(r"resumed=\S+ \| pose/max_offset=(\S+)\n", out2)
    assert m and abs(float(m.group(1)) - want) <= 1e-5 * want + 1e-9, out2
