"""GPU: the launcher's mesh simplification (eonerf_code_amd/train_dp.py --mesh_out PATH --mesh_simplify K): the status line shows the
vertex and face counts before and after, the PLY holds the simplified mesh with normals and albedo at its vertices, and mesh/mae= is of
that mesh.  One run; the scene and the step count are those of tests/test_train_dp_mesh_dsm_gpu.py."""
import math
import os
import re

import pytest
import torch

import mesh_restated as mr
from test_train_dp_mesh_dsm_gpu import RES, run

pytestmark = pytest.mark.gpu


def test_launcher_saves_the_simplified_mesh_and_scores_it(tmp_path):
    H = 32
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="ij")
    gt_path = os.path.join(str(tmp_path), "gt.pt")
    torch.save({"dsm": 30 + 6 * torch.sin(xx / 5) * torch.cos(yy / 7), "roi": [1000.0, 5000.0, float(H), 0.5], "scene_offset": [1008.0, 5008.0, 30.0],
                "scene_scale": [8.0, 8.0, 40.0], "sun": [35.0, 160.0]}, gt_path)
    ply = str(tmp_path / "a" / "scene.ply")
    out = run(tmp_path / "logs", ["--mesh_out", ply, "--gt_dsm", gt_path, "--mesh_res", str(RES), "--mesh_level", "0.3", "--mesh_simplify", "2",
                                  "--mesh_representative", "nearest"])
    line = re.findall(r"mesh=\S+ \| vertices=(\d+) \| faces=(\d+) \| level=\S+ \| vertices_in=(\d+) \| faces_in=(\d+)", out)
    assert len(line) == 1, out
    n_v, n_f, v_in, f_in = (int(x) for x in line[0])
    print(f"vertices {v_in} -> {n_v}, faces {f_in} -> {n_f}")
    assert 0 < n_v < v_in and 0 < n_f < f_in
    got = mr.read_ply(ply)
    assert len(got["x"]) == n_v and got["faces"].shape == (n_f, 3) and got["faces"].min() >= 0 and got["faces"].max() < n_v
    assert "nx" in got and "red" in got
    found = re.findall(r"mesh/mae=(\S+) \| mesh/cells=(\d+)", out)
    assert len(found) == 1 and math.isfinite(float(found[0][0])) and int(found[0][1]) > 0, out
