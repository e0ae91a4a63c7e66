"""GPU: the launcher's mesh export (eonerf_code_amd/train_dp.py --mesh_out PATH --mesh_res N --mesh_level L): after the last step rank 0
writes a readable PLY; without the flag there is no file, and the final checkpoint and the final parameters are the same bits."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_restated as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 17


def run(logs, extra):
    # 2048 rays / 512 per step = 4 steps per epoch; a checkpoint is due every 4 epochs: step 16 is the last step and writes one
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "512", "--n_images", "2",
           "--n_samples", "64", "--max_train_steps", "16", "--check_every", "8", "--logs_dir", str(logs), "--exp_name", "t",
           "--dump_params", os.path.join(str(logs), "params")] + extra
    # fixed-order gradient sums: two runs then hold the same weights bit for bit
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), EONERF_DETERMINISTIC="1")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and a.reshape(-1).contiguous().view(torch.uint8).equal(b.reshape(-1).contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_launcher_writes_a_readable_ply_and_leaves_the_run_alone(tmp_path):
    flagged, plain = tmp_path / "flagged", tmp_path / "plain"
    ply = str(tmp_path / "out" / "scene.ply")
    # a level inside the density range of a field sixteen steps old (the default is far above it): 962 vertices, 1,522 faces when measured
    out = run(flagged, ["--mesh_out", ply, "--mesh_res", str(RES), "--mesh_level", "0.3"])
    m = re.search(r"mesh=\S+ \| vertices=(\d+) \| faces=(\d+) \| level=0\.3", out)
    assert m and os.path.exists(ply), out
    print(m.group(0))
    got = mr.read_ply(ply)
    assert sorted(got) == ["blue", "faces", "green", "nx", "ny", "nz", "red", "x", "y", "z"]
    assert len(got["x"]) == int(m.group(1)) and len(got["faces"]) == int(m.group(2))
    xyz = np.stack([got["x"], got["y"], got["z"]], 1)
    assert xyz.dtype == np.float32 and np.isfinite(xyz).all() and (np.abs(xyz) <= 1).all()
    assert len(got["faces"]) > 0 and got["faces"].min() >= 0 and got["faces"].max() < len(xyz)
    most, _ = mr.edge_report(got["faces"])
    assert most == 1
    normals = np.stack([got["nx"], got["ny"], got["nz"]], 1)
    lengths = np.linalg.norm(normals, axis=1)
    assert (np.abs(lengths[lengths > 0] - 1) <= 1e-5).all() and (lengths > 0).any()
    without = run(plain, [])
    assert "mesh=" not in without
    assert [p for p in glob.glob(os.path.join(str(plain), "**", "*"), recursive=True) if p.endswith(".ply")] == []
    ck_a, ck_b = (sorted(glob.glob(os.path.join(str(d), "t", "ckpts", "*.ckpt"))) for d in (flagged, plain))
    assert len(ck_a) == 1 and [os.path.basename(p) for p in ck_a] == [os.path.basename(p) for p in ck_b]
    a, b = (torch.load(p[-1], map_location="cpu", weights_only=False) for p in (ck_a, ck_b))
    assert same(a, b) and len(a["model_state_dict"]) > 10
    pa, pb = (torch.load(os.path.join(str(d), "params.rank0"), map_location="cpu") for d in (flagged, plain))
    assert same(pa, pb)
    losses = lambda text: re.findall(r"step=(\d+) \| loss=([^\s|]+)", text)       # noqa: E731
    assert losses(out) == losses(without) and len(losses(out)) == 3
