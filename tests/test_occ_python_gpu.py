"""GPU: the occupancy grid through the Python layer (eonerf_code_amd/occupancy.py, render_image, checkpoints, train_dp.py --occ_grid).
The culling rule itself is pinned at the C ABI (tests/test_occ_gpu.py); here: which calls honour a grid, and that it travels."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import eonerf_oracle as orc
import occ_restated as occ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IMG, R, S = 4, 67, 37
STEP = 2.0 / S


def _state(seed=5):
    sd = orc.random_state_dict(N_IMG, seed=seed, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    return sd


def _field(sd, precision="bf16", eval_precision=None):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision=precision, eval_precision=eval_precision)
    f.load_state_dict(sd)
    return f.cuda()


def _slab_grid(r=5, dilate=False):
    """OccupancyGrid with only the cells iz < r // 4 set."""
    from eonerf_code_amd.occupancy import OccupancyGrid, bits_from_binaries
    g = OccupancyGrid(r, device="cuda")
    g.bits = bits_from_binaries((torch.arange(r, device="cuda")[None, None, None, :] < r // 4).expand(1, r, r, r))
    g.dilate, g._export_bits = dilate, None
    return g


def _render(f, grid, eval=True, seed=9):
    from eonerf_code_amd.sat_rendering import render_image
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    rays, ts, _, u_cam, u_sun = orc.synthetic_batch(R, N_IMG, seed=seed, n_samples=S)
    sr = define_satrays_from_tensors(rays.cuda(), ts.cuda())
    return render_image(f, grid, sr, None, None, epoch_idx=3, chunk=R, render_step_size=STEP, noise=[(u_cam, None, u_sun)], eval=eval)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b)


def test_render_image_honours_a_grid_on_export_renders_only():
    from eonerf_code_amd.occupancy import OccupancyGrid
    f = _field(_state())
    with torch.no_grad():
        plain, n_plain = _render(f, None)
        ones, n_ones = _render(f, OccupancyGrid(5))                      # a new grid is all ones: the identity, bit for bit
        assert n_ones == n_plain and _same(ones, plain)
        other, n_other = _render(f, object())                             # anything else is ignored, as it always was
        assert n_other == n_plain and _same(other, plain)
        culled, n_culled = _render(f, _slab_grid())
        assert n_culled < n_plain and not torch.equal(culled["depth"], plain["depth"])
        assert float(culled["pts_per_ray"].sum()) == n_culled            # the kept counts (no ray is empty here: no retry)
        dilated, n_dilated = _render(f, _slab_grid(dilate=True))          # one cell of margin keeps more
        assert n_culled < n_dilated < n_plain
        assert _same(_render(f, None)[0], plain)                          # nothing stays on the context
    # a training call ignores the grid
    f.train()
    a, n_a = _render(f, None, eval=False)
    b, n_b = _render(f, _slab_grid(), eval=False)
    assert a["rgb"].requires_grad and n_a == n_b and _same(b, a)


def test_a_grid_built_for_another_step_size_is_refused():
    f = _field(_state())
    g = _slab_grid()
    g.render_step_size = STEP / 2.5
    with torch.no_grad(), pytest.raises(ValueError, match="factor of 2"):
        _render(f, g)
    g.render_step_size = STEP / 2
    with torch.no_grad():
        _render(f, g)


def test_the_fp32_retry_of_an_out_of_range_export_keeps_the_grid():
    sd = {k: v.clone() for k, v in _state().items()}
    for k in (1, 2, 3):      # X_4 reaches ~1e6 (> 65504): the kernels' activation probe fires (tests/test_f16x3_range.py)
        sd[f"base_mlp.hidden_layers.{k}.weight"] *= 400.0
    f = _field(sd)
    assert f.eval_precision == "fp16x3"
    g = _slab_grid()
    with warnings.catch_warnings(record=True) as w, torch.no_grad():
        warnings.simplefilter("always")
        got, n = _render(f, g)
    assert any("fp16x3" in str(x.message) for x in w) and f.eval_precision == "fp32"
    with torch.no_grad():
        f32 = _field(sd, eval_precision="fp32")
        want, n32 = _render(f32, g)
        plain, n_plain = _render(f32, None)
    assert n == n32 and _same(got, want)      # the retry culled by the same grid on the fp32 context
    assert n < n_plain


def test_update_build_and_dilation_on_the_device():
    from eonerf_code_amd.occupancy import OccupancyGrid, binaries_from_bits
    f = _field(_state())
    g = OccupancyGrid(32)
    assert g.update_every_n_steps(7, f, STEP) is False and bool(g.binaries.all())
    assert g.update_every_n_steps(50, f, STEP, occ_thre=1.0) is True      # thr = the mean: some cells above, some below
    b = g.binaries
    assert b.shape == (1, 32, 32, 32) and 0 < int(b.sum()) < 32 ** 3
    assert float(g.threshold[0]) == pytest.approx(float(g.occs.double().mean()), rel=1e-6)
    assert g.render_step_size == STEP
    g.build(f, STEP, passes=3, occ_thre=1.0)
    raw = g.binaries.cpu().numpy().reshape(-1)
    export = binaries_from_bits(g.export_bits, 32).cpu().numpy().reshape(-1)
    assert np.array_equal(export, occ.dilate(raw, 32)) and export.sum() > raw.sum()
    g.build(f, STEP, passes=1, occ_thre=1.0, dilate=False)
    assert g.export_bits is g.bits
    h = OccupancyGrid(32)
    h.load_state_dict(g.state_dict())
    assert torch.equal(h.bits, g.bits) and torch.equal(h.occs, g.occs)


def test_launcher_with_occ_grid_validates_with_it_and_checkpoints_it(tmp_path):
    from eonerf_code_amd.checkpoint import load_checkpoint
    from eonerf_code_amd.occupancy import OccupancyGrid
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    from eonerf_code_amd.synthetic import synthetic_batch
    rays, _, rgbs = synthetic_batch(12 * 10, 5, seed=77)
    val = os.path.join(str(tmp_path), "val.pt")
    torch.save({"images": [{"rays": rays, "rgbs": rgbs, "h": 12, "w": 10}]}, val)
    # 2048 rays / 1024 per step = 2 steps per epoch: the launcher's periodic save (every fourth epoch) writes at step 8, the first step
    # of epoch 4, behind the grid updates of steps 0, 4 and 8 and the validations of epochs 0 .. 3; step 9 ends the run
    cmd = [sys.executable, "-m", "eonerf_code_amd.train_dp", "--synthetic_rays", "2048", "--batch_size", "1024", "--n_images", "5",
           "--max_train_steps", "9", "--logs_dir", str(tmp_path), "--exp_name", "t", "--occ_grid", "--occ_every", "4", "--val_images", val]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("val/psnr=") == 4, r.stdout
    path = os.path.join(str(tmp_path), "t", "ckpts", "epoch=4.ckpt")
    ck = torch.load(path, weights_only=False)
    sd = ck["occ_grid_state_dict"]
    assert list(sd.keys()) == ["resolution", "aabbs", "occs", "binaries"] and sd["resolution"].tolist() == [128, 128, 128]
    frac = float(sd["binaries"].float().mean())
    print(f"checkpointed grid: {frac:.4f} of the cells set, max occ {float(sd['occs'].max()):.4g}")
    assert 0 < frac < 1 and float(sd["occs"].max()) > 0
    g = OccupancyGrid(128)
    f = EONerfMLP(5, radiometric_normalization=True, precision="bf16").cuda()
    assert load_checkpoint(path, f, occ_grid=g) == 4
    assert torch.equal(g.binaries.cpu(), sd["binaries"]) and torch.equal(g.occs.cpu(), sd["occs"])
    with torch.no_grad():      # ... and renders cull by it
        from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
        from eonerf_code_amd.sat_rendering import render_image
        sr = define_satrays_from_tensors(rays.cuda(), torch.zeros(rays.shape[0], 1, dtype=torch.int64, device="cuda"))
        f.eval()
        _, n_grid = render_image(f, g, sr, None, None, epoch_idx=3, chunk=4096, render_step_size=2.0 / 128)
        _, n_plain = render_image(f, None, sr, None, None, epoch_idx=3, chunk=4096, render_step_size=2.0 / 128)
    assert n_grid < n_plain
