"""GPU: the launcher's mesh views (eonerf_code_amd/train_dp.py --mesh_out PATH --val_images FILE --mesh_views): after the mesh is saved
rank 0 casts every held-out image's rays against it and prints mesh/view_depth=, mesh/view_hits= and mesh/shadow_agree= once; without
the flag the same run prints none of them and leaves the same checkpoint and weights; the flag alone is refused.  The scene and the
step count are those of tests/test_train_dp_mesh_gpu.py (fixed-order gradient sums: both runs hold the same weights)."""
import glob
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from test_train_dp_mesh_gpu import RES, ROOT, run, same

pytestmark = pytest.mark.gpu
SIZES = [(12, 10), (9, 11)]


def val_file(tmp_path):
    from eonerf_code_amd.synthetic import synthetic_batch
    images = []
    for k, (h, w) in enumerate(SIZES):
        rays, _, rgbs = synthetic_batch(h * w, 2, seed=77 + k)
        images.append({"rays": rays, "rgbs": rgbs, "h": h, "w": w})
    path = os.path.join(str(tmp_path), "val.pt")
    torch.save({"images": images}, path)
    return path


def test_launcher_prints_the_three_keys_with_the_flag_and_nothing_new_without_it(tmp_path):
    path = val_file(tmp_path)
    flagged, plain = tmp_path / "flagged", tmp_path / "plain"
    common = ["--mesh_res", str(RES), "--mesh_level", "0.3", "--val_images", path]
    out = run(flagged, ["--mesh_out", str(tmp_path / "a" / "scene.ply"), "--mesh_views"] + common)
    found = re.findall(r"mesh/view_depth=(\S+) \| mesh/view_hits=(\d+) \| mesh/view_rays=(\d+) \| mesh/shadow_agree=(\S+)\n", out)
    assert len(found) == 1, out
    print("mesh/view_depth=%s mesh/view_hits=%s mesh/view_rays=%s mesh/shadow_agree=%s" % found[0])
    depth, hits, rays, agree = float(found[0][0]), int(found[0][1]), int(found[0][2]), float(found[0][3])
    assert rays == sum(h * w for h, w in SIZES) and 0 <= hits <= rays
    assert math.isfinite(depth) and depth >= 0 and 0.0 <= agree <= 1.0
    assert out.index("mesh=") < out.index("mesh/view_depth=")                 # after the mesh is saved
    without = run(plain, ["--mesh_out", str(tmp_path / "b" / "scene.ply")] + common)
    assert "mesh/view" not in without and "mesh/shadow_agree" not in without and "mesh=" in without
    strip = lambda text: re.sub(r"elapsed_time=[\d.]+s|rays/s=\d+|mesh=\S+", "", "".join(l for l in text.splitlines(True) if "mesh/view_depth=" not in l))    # noqa: E731
    assert strip(out) == strip(without)
    ck_a, ck_b = (sorted(glob.glob(os.path.join(str(d), "t", "ckpts", "*.ckpt"))) for d in (flagged, plain))
    assert len(ck_a) == 1 and [os.path.basename(p) for p in ck_a] == [os.path.basename(p) for p in ck_b]
    a, b = (torch.load(p[-1], map_location="cpu", weights_only=False) for p in (ck_a, ck_b))
    assert same(a, b) and len(a["model_state_dict"]) > 10
    pa, pb = (torch.load(os.path.join(str(d), "params.rank0"), map_location="cpu") for d in (flagged, plain))
    assert same(pa, pb)
    assert open(str(tmp_path / "a" / "scene.ply"), "rb").read() == open(str(tmp_path / "b" / "scene.ply"), "rb").read()


def test_launcher_refuses_the_flag_alone(tmp_path):
    path = val_file(tmp_path)
    for extra in (["--mesh_views"], ["--mesh_views", "--val_images", path], ["--mesh_views", "--mesh_out", str(tmp_path / "x.ply")]):
        cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "512", "--n_images", "2", "--max_train_steps", "1",
               "--logs_dir", str(tmp_path / "logs"), "--exp_name", "t"] + extra
        r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")), capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--mesh_views" in r.stderr and "--mesh_out" in r.stderr and "--val_images" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(str(tmp_path / "x.ply")) and not os.path.exists(str(tmp_path / "logs"))
