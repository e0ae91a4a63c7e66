"""GPU: early ray termination through the Python layer (render_image(early_stop_eps=, march_block=), validate_images, evaluate_dsm).
The rule itself is pinned at the C ABI (tests/test_march_gpu.py); here: which calls honour the knob, that an export render is the
C entry point chunk by chunk, and that the arguments travel."""
import ctypes as C

import pytest
import torch

from oracle import eonerf_oracle as orc

pytestmark = pytest.mark.gpu
N_IMG, R, S, CHUNK = 4, 67, 37, 30      # chunks of 30, 30 and a ragged 7
STEP = 2.0 / S
SHADOWS, EVAL = 1, 2


def _state(seed=5):
    sd = orc.random_state_dict(N_IMG, seed=seed, bias_scale=0.05)
    sd["sigma_layer.output_layer.bias"] += 1.0
    return sd


def _field(precision="bf16", eval_precision=None):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision=precision, eval_precision=eval_precision)
    f.load_state_dict(_state())
    return f.cuda()


def _batch():
    rays, ts, _, u_cam, u_sun = orc.synthetic_batch(R, N_IMG, seed=9, n_samples=S)
    rays[:, 2] = 0.98 + 0.11 * (torch.arange(R) % 13).float()      # rays enter the cube at different slots (tests/test_march_gpu.py)
    u_retry = torch.rand(R, S, generator=torch.Generator().manual_seed(999))
    return rays.cuda(), ts.cuda(), u_cam.cuda(), u_retry.cuda(), u_sun.cuda()


def _render(f, eval=True, **kw):
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
    from eonerf_code_amd.sat_rendering import render_image
    rays, ts, u_cam, u_retry, u_sun = _batch()
    noise = [(u_cam[i:i + CHUNK], u_retry[i:i + CHUNK], u_sun[i:i + CHUNK]) for i in range(0, R, CHUNK)]
    return render_image(f, None, define_satrays_from_tensors(rays, ts), None, None, epoch_idx=3, chunk=CHUNK, render_step_size=STEP, noise=noise,
                        eval=eval, **kw)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("block", [16, 32])
def test_an_export_render_with_early_stop_eps_is_the_c_entry_point_chunk_by_chunk(block):
    from eonerf_code_amd import _lib
    from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors, satrays_to_table
    from eonerf_code_amd.sat_rendering import RESULT_SLICES, _zsteps
    f = _field()
    eps = 0.25
    with torch.no_grad():
        got, n_got = _render(f, early_stop_eps=eps, march_block=block)
        plain, n_plain = _render(f)
    rays, ts, u_cam, u_retry, u_sun = _batch()
    table, img = satrays_to_table(define_satrays_from_tensors(rays, ts))
    native, flat = f._native(True)      # the export context render_image ran on
    L = _lib.lib()
    P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    outs, total = [], 0
    for i in range(0, R, CHUNK):
        t, im = table[i:i + CHUNK].contiguous(), img[i:i + CHUNK].contiguous()
        n = t.shape[0]
        nb = L.eonerf_march_workspace_bytes(native, n, SHADOWS | EVAL, block)
        ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        out = torch.full((n, 21), float("nan"), device="cuda")
        cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = L.eonerf_render_forward_march(native, P(flat), P(t), P(im), P(_zsteps(t.device, S)), P(u_cam[i:i + CHUNK].contiguous()),
                                           P(u_retry[i:i + CHUNK].contiguous()), P(u_sun[i:i + CHUNK].contiguous()), n, SHADOWS | EVAL,
                                           C.c_float(eps), block, P(out), P(cnt), None, P(ws), nb, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append(out)
        total += int(cnt[0])
    want = torch.cat(outs)
    for k, a, b in RESULT_SLICES:
        assert torch.equal(got[k].reshape(R, -1).view(torch.int32), want[:, a:b].contiguous().view(torch.int32)), k
    assert n_got == total < n_plain      # the kept camera samples; the march dropped some
    assert torch.equal(got["pts_per_ray"], plain["pts_per_ray"])      # columns 14 stays the full count
    assert not torch.equal(got["depth"], plain["depth"])
    assert (got["depth"] - plain["depth"]).abs().max().item() <= 2 * eps + 2e-4      # against the DENSE render: the bound against eps = 0, which is within 1e-4 of it


def test_training_calls_and_eps_zero_run_the_existing_entry_point():
    f = _field()
    with torch.no_grad():
        plain, n_plain = _render(f)
        zero, n_zero = _render(f, early_stop_eps=0.0, march_block=16)
        assert n_zero == n_plain and _same(zero, plain)
        f.eval()
        modal, n_modal = _render(f, eval=False, early_stop_eps=0.25)      # .eval() mode under no_grad: an export render too
        base, n_base = _render(f, eval=False)
        assert n_modal < n_base
        f.train()
        with pytest.raises(ValueError, match="16, 32 or 64"):
            _render(f, early_stop_eps=0.25, march_block=48)
    # a training call ignores the knob
    a, n_a = _render(f, eval=False)
    b, n_b = _render(f, eval=False, early_stop_eps=0.25)
    assert a["rgb"].requires_grad and b["rgb"].requires_grad and n_a == n_b and _same(b, a)
    # ... as does a module in train mode under no_grad (not an export render)
    with torch.no_grad():
        c, n_c = _render(f, eval=False, early_stop_eps=0.25)
        d, n_d = _render(f, eval=False)
    assert n_c == n_d and _same(c, d)


def test_the_fp32_retry_of_an_out_of_range_export_marches_too():
    import warnings
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    sd = {k: v.clone() for k, v in _state().items()}
    for k in (1, 2, 3):      # X_4 reaches ~1e6 (> 65504): the kernels' activation probe fires (tests/test_f16x3_range.py)
        sd[f"base_mlp.hidden_layers.{k}.weight"] *= 400.0

    def field(eval_precision=None):
        f = EONerfMLP(N_IMG, radiometric_normalization=True, precision="bf16", eval_precision=eval_precision)
        f.load_state_dict(sd)
        return f.cuda()

    f = field()
    assert f.eval_precision == "fp16x3"
    with warnings.catch_warnings(record=True) as w, torch.no_grad():
        warnings.simplefilter("always")
        got, n = _render(f, early_stop_eps=0.25)
    assert any("fp16x3" in str(x.message) for x in w) and f.eval_precision == "fp32"
    with torch.no_grad():
        want, n32 = _render(field("fp32"), early_stop_eps=0.25)
    assert n == n32 and _same(got, want)


class _Seen(Exception):
    pass


def test_validate_images_and_evaluate_dsm_forward_the_arguments(monkeypatch):
    from eonerf_code_amd import dsm, sat_rendering, validation
    f = _field()
    rays, ts, _, _, _ = _batch()
    h, w = 6, 5
    image = {"rays": rays[:h * w].contiguous(), "rgbs": torch.rand(h * w, 3, generator=torch.Generator().manual_seed(1)).cuda(), "h": h, "w": w}
    real, seen = sat_rendering.render_image, []

    def spy(*a, **k):
        seen.append(k)
        return real(*a, **k)

    monkeypatch.setattr(sat_rendering, "render_image", spy)
    f.set_noise_seed(7)
    dense, _ = validation.validate_images(f, [image], 3, chunk=16, render_step_size=STEP)
    f.set_noise_seed(7)
    table, _ = validation.validate_images(f, [image], 3, chunk=16, render_step_size=STEP, early_stop_eps=0.6, march_block=16)
    assert seen[0]["early_stop_eps"] == 0.0 and seen[0]["march_block"] == 32
    assert seen[1]["early_stop_eps"] == 0.6 and seen[1]["march_block"] == 16
    assert bool(torch.isfinite(table[:, :5]).all()) and not torch.equal(table[:, :5], dense[:, :5])      # the marched render is another image

    def stop(*a, **k):
        seen.append(k)
        raise _Seen

    monkeypatch.setattr(sat_rendering, "render_image", stop)
    gt = torch.zeros(8, 8, device="cuda")
    with pytest.raises(_Seen):
        dsm.evaluate_dsm(f, gt, (0.0, 0.0, 8, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (40.0, 120.0), early_stop_eps=1e-3, march_block=64)
    assert seen[-1]["early_stop_eps"] == 1e-3 and seen[-1]["march_block"] == 64 and seen[-1]["only_depth"] is True
    with pytest.raises(_Seen):
        dsm.evaluate_dsm(f, gt, (0.0, 0.0, 8, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (40.0, 120.0))
    assert seen[-1]["early_stop_eps"] == 0.0 and seen[-1]["march_block"] == 32
