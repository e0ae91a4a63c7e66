"""GPU: the launcher's true orthophoto (eonerf_code_amd/train_dp.py --ortho FILE --ortho_out PATH): after the last step rank 0 gathers
the input images on the rendered nadir surface and saves the mosaic with its geotransform; without the flag the launcher's status
lines are what they were."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ortho_restated as OR
from oracle import raygen_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, IMG = 12, 10, 16


def run(tmp_path, extra):
    # 2048 rays / 512 per step = 4 steps per epoch; 5 steps = epoch 0 complete, one step of epoch 1
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "512", "--n_images", "2",
           "--n_samples", "64", "--max_train_steps", "5", "--check_every", "2", "--logs_dir", str(tmp_path), "--exp_name", "t"] + extra
    # fixed-order gradient sums: two runs then print the same losses digit for digit
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), EONERF_DETERMINISTIC="1")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_launcher_saves_the_orthophoto_and_leaves_the_loss_lines_alone(tmp_path):
    rng = np.random.default_rng(3)
    zone, south, offset = OR.scene_frame(30.33)
    rpcs = [RO.rescale_rpc(RO.synthetic_rpc(50 + k, lat0=30.33, lon0=OR.LON0), IMG / 2048.0) for k in range(2)]
    images = [torch.from_numpy(rng.uniform(0, 1, (IMG, IMG, 3)).astype(np.float32)) for _ in range(2)]
    src, dst = os.path.join(str(tmp_path), "ortho_in.pt"), os.path.join(str(tmp_path), "out", "ortho.pt")
    torch.save({"images": images, "rpcs": rpcs, "size": [H, W], "min_alt": -10.0, "max_alt": 50.0, "scene_offset": offset.tolist(),
                "scene_scale": list(OR.SCENE_SCALE), "zone": zone, "south": south}, src)
    with_flag = run(tmp_path, ["--ortho", src, "--ortho_out", dst])
    assert os.path.exists(dst) and re.search(r"ortho=\S+ \| cells=\d+/%d" % (H * W), with_flag), with_flag
    d = torch.load(dst, map_location="cpu")
    assert d["mosaic"].shape == (H, W, 3) and d["count"].shape == (H, W) and d["weight"].shape == (H, W)
    seen = d["count"] > 0
    assert torch.isfinite(d["mosaic"][seen]).all() and torch.isnan(d["mosaic"][~seen]).all()
    from eonerf_code_amd.ortho import nadir_geotransform
    assert tuple(d["geotransform"]) == nadir_geotransform(H, W, offset, OR.SCENE_SCALE)
    # without the flag: no file, no ortho line, and the same loss= lines (the orthophoto runs after the last step has been taken)
    without = run(tmp_path, [])
    assert "ortho=" not in without and not os.path.exists(os.path.join(str(tmp_path), "t", "ortho.pt"))
    losses = lambda out: re.findall(r"step=(\d+) \| loss=([^\s|]+)", out)       # noqa: E731
    assert losses(with_flag) == losses(without) and len(losses(without)) == 3
