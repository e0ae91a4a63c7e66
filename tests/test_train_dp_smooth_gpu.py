"""GPU: the launcher's mesh smoothing (eonerf_code_amd/train_dp.py --mesh_out PATH --mesh_smooth K): the status line ends in smooth=K and
the number of open vertices, the PLY holds the unsmoothed run's vertices and faces in number and order -- the same faces, moved vertices
-- and mesh/mae= is of that mesh.  The scene and the step count are those of tests/test_train_dp_mesh_dsm_gpu.py; the second run, without
the flag, is what the first is compared with (fixed-order gradient sums: both hold the same weights)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_restated as mr
from test_train_dp_mesh_dsm_gpu import RES, run

pytestmark = pytest.mark.gpu


def test_launcher_saves_the_smoothed_mesh_and_scores_it(tmp_path):
    H = 32
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    gt_path = os.path.join(str(tmp_path), "gt.pt")
    torch.save({"dsm": 30 + 6 * torch.sin(xx / 5) * torch.cos(yy / 7), "roi": [1000.0, 5000.0, float(H), 0.5], "scene_offset": [1008.0, 5008.0, 30.0],
                "scene_scale": [8.0, 8.0, 40.0], "sun": [35.0, 160.0]}, gt_path)
    ply, plain_ply = str(tmp_path / "a" / "smooth.ply"), str(tmp_path / "a" / "plain.ply")
    common = ["--gt_dsm", gt_path, "--mesh_res", str(RES), "--mesh_level", "0.3"]
    out = run(tmp_path / "logs", ["--mesh_out", ply, "--mesh_smooth", "3"] + common)
    line = re.findall(r"mesh=\S+ \| vertices=(\d+) \| faces=(\d+) \| level=\S+ \| smooth=(\d+) \| open=(\d+)", out)
    assert len(line) == 1, out
    n_v, n_f, k, n_open = (int(x) for x in line[0])
    assert k == 3 and 0 <= n_open <= n_v and n_v > 0 and n_f > 0
    found = re.findall(r"mesh/mae=(\S+) \| mesh/cells=(\d+)", out)
    assert len(found) == 1 and math.isfinite(float(found[0][0])) and int(found[0][1]) > 0, out
    plain_out = run(tmp_path / "logs2", ["--mesh_out", plain_ply] + common)
    assert "smooth=" not in plain_out
    got, plain = mr.read_ply(ply), mr.read_ply(plain_ply)
    assert len(got["x"]) == len(plain["x"]) == n_v and got["faces"].shape == plain["faces"].shape == (n_f, 3)
    assert np.array_equal(got["faces"], plain["faces"]) and "nx" in got and "red" in got
    a, b = np.stack([got["x"], got["y"], got["z"]], 1), np.stack([plain["x"], plain["y"], plain["z"]], 1)
    moved = (a != b).any(axis=1)
    print(f"{n_v} vertices, {n_f} faces, {n_open} open, {int(moved.sum())} moved")
    assert moved.any() and int(moved.sum()) <= n_v - n_open and np.isfinite(a).all()
