"""GPU: eonerf_render_origin_grad (include/eonerf_pose.h) -- d loss / d ray origin of a training step and its per-image sum, at the C ABI.

Yardstick: the restatement's own autograd with respect to the ray table (columns 0..2 of rays.grad), in fp32 and fp64, under the
project's fp32 criterion (tests/test_hip_backward.py):  |hip - fp64| <= 1.5 |ref32 - fp64| + 2e-3 |fp64|  in L2, applied to d_origins as
a whole and to d_offsets (= index_add of the reference rows).  Measured ratios err / (ref_err + 2e-3 |fp64|) are printed by every case.
"""
import ctypes as C

import pytest
import torch

from oracle import eonerf_oracle as orc
from workspace_guard import Guarded, assert_same_bits, check_guards

pytestmark = pytest.mark.gpu
EXACT_FACTOR = 1.5
E_ARG, E_WORKSPACE, E_STATE, E_UNSUPPORTED = -1, -2, -3, -4
N_IMG, R = 6, 192
_CACHE = {}


def base_case():
    """Field and batch of test_backward_fp32_random_batch_all_parameters."""
    if "base" not in _CACHE:
        sd = orc.random_state_dict(N_IMG, seed=51, bias_scale=0.05, radiometric_jitter=0.05)
        sd["sigma_layer.output_layer.bias"] += 1.0
        _CACHE["base"] = (sd,) + tuple(orc.synthetic_batch(R, N_IMG, seed=52))
    return _CACHE["base"]


def make_field(sd, n_img, precision):
    from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
    f = EONerfMLP(n_img, radiometric_normalization=True, precision=precision)
    f.load_state_dict(sd, strict=True)
    return f.cuda()


def reference(sd, rays, ts, rgbs, u_cam, u_sun, epoch, step, dtype, u_retry=None):
    """(loss, d loss / d origins [R, 3], its per-image sum [n_img, 3]) of the restatement's autograd in `dtype`."""
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    r = cast(rays).clone().requires_grad_(True)
    field = orc.Field({k: cast(v) for k, v in sd.items()})
    out, _ = orc.render_rays(field, orc.define_satrays_from_tensors(r, ts), cast(u_cam), cast(u_sun), epoch, step,
                             u_cam_retry=None if u_retry is None else cast(u_retry))
    loss = orc.train_loss(out, cast(rgbs), epoch)
    loss.backward()
    g = r.grad[:, :3].detach()
    n_img = sd["transient_encoder.weight"].shape[0]
    return loss.detach(), g, torch.zeros(n_img, 3, dtype=dtype).index_add_(0, ts.reshape(-1), g)


class Abi:
    """One training step through the C ABI on buffers the test owns: forward, fused loss + backward, then (optionally) the origin gradient."""

    def __init__(self, f, n, ns=128):
        from eonerf_code_amd import _lib
        from eonerf_code_amd._lib import _ptr, _stream
        from eonerf_code_amd.sat_rendering import _zsteps
        self.lib, self.L, self.ptr, self.stream = _lib, _lib.lib(), _ptr, _stream
        self.f, self.n, self.ns = f, n, ns
        self.ctx = f._context()
        self.flat = f._ensure_packed()
        f.set_n_samples(ns)
        self.z = _zsteps(self.flat.device, ns)
        self.n_images = f.n_input_images

    def ws_bytes(self, flags, n=None):
        return self.L.eonerf_render_workspace_bytes(self.ctx, self.n if n is None else n, flags)

    def step(self, rays, img, rgbs, noise, flags, kind, ws=None):
        L, p, dev = self.L, self.ptr, self.flat.device
        n = rays.shape[0]
        self.rays, self.img = rays.cuda().contiguous(), img.reshape(-1).cuda().contiguous()
        self.flags = flags
        self.ws = torch.empty(self.ws_bytes(flags, n), dtype=torch.uint8, device=dev) if ws is None else ws
        self.out = torch.empty(n, 21, dtype=torch.float32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        u = [None if t is None else t.cuda().float().contiguous() for t in noise]
        if not flags & self.lib.F_SHADOWS:
            u[2] = None
        self._keep = u
        self.lib.check(L.eonerf_render_forward(self.ctx, p(self.flat), p(self.rays), p(self.img), p(self.z), p(u[0]), p(u[1]), p(u[2]), n, flags,
                                               p(self.out), p(cnt), p(self.ws), self.ws.numel(), self.stream()))
        self.d_flat = torch.zeros(L.eonerf_grad_floats(self.ctx), dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        d_out = torch.zeros(n, 21, dtype=torch.float32, device=dev)
        pix = rgbs.cuda().float().contiguous()
        self.lib.check(L.eonerf_render_backward_loss(self.ctx, p(self.flat), p(self.rays), p(self.img), n, flags, p(self.out), p(pix), kind, p(d_out),
                                                     p(self.loss), p(self.d_flat), p(self.ws), self.ws.numel(), self.stream()))
        return self

    def scratch_bytes(self, n=None):
        return self.L.eonerf_origin_grad_scratch_bytes(self.ctx, self.rays.shape[0] if n is None else n, self.flags)

    def origin_grad_rc(self, d_origins, d_offsets, scratch, scratch_bytes=None, n=None, flags=None):
        p = self.ptr
        ptr_of = lambda t: (C.c_void_p(t.ptr) if isinstance(t, Guarded) else p(t))
        return self.L.eonerf_render_origin_grad(self.ctx, p(self.flat), p(self.rays), p(self.img), self.rays.shape[0] if n is None else n,
                                                self.flags if flags is None else flags, p(self.ws), self.ws.numel(), ptr_of(scratch),
                                                (scratch.nbytes if isinstance(scratch, Guarded) else scratch.numel()) if scratch_bytes is None else scratch_bytes,
                                                ptr_of(d_origins), ptr_of(d_offsets), self.stream())

    def origin_grad(self, d_offsets=None):
        dev = self.flat.device
        d_origins = torch.full((self.rays.shape[0], 3), float("nan"), dtype=torch.float32, device=dev)
        if d_offsets is None:
            d_offsets = torch.zeros(self.n_images, 3, dtype=torch.float32, device=dev)
        scratch = torch.empty(self.scratch_bytes(), dtype=torch.uint8, device=dev)
        self.lib.check(self.origin_grad_rc(d_origins, d_offsets, scratch))
        return d_origins, d_offsets


def flags_of(tag):
    from eonerf_code_amd import _lib
    return {"e0_rgb": (_lib.F_TRAIN | _lib.F_RGB_LOSS, 0, 0), "e0": (_lib.F_TRAIN, 0, 0), "e3": (_lib.F_TRAIN | _lib.F_SHADOWS, 1, 3)}[tag]


def exactness(tag, got, r32, r64):
    got, r32 = got.double().cpu(), r32.double()
    ref_err, err, scale = (r32 - r64).norm().item(), (got - r64).norm().item(), r64.norm().item()
    ratio = err / (ref_err + 2e-3 * scale + 1e-12)
    print(f"origin-grad exactness {tag}: err={err:.3e} ref_err={ref_err:.3e} |fp64|={scale:.3e} ratio={ratio:.3f}")
    assert err <= EXACT_FACTOR * ref_err + 2e-3 * scale + 1e-12, (tag, err, ref_err, scale)
    return ratio


def check_against_reference(tag, sd, rays, ts, rgbs, u_cam, u_sun, step, ns, u_retry=None, d_offsets=None):
    flags, kind, epoch = flags_of(tag.split(":")[0])
    f = make_field(sd, sd["transient_encoder.weight"].shape[0], "fp32")
    a = Abi(f, rays.shape[0], ns).step(rays, ts, rgbs, (u_cam, u_retry, u_sun), flags, kind)
    pre = None if d_offsets is None else d_offsets.clone()
    d_origins, d_off = a.origin_grad(d_offsets)
    l32, g32, o32 = reference(sd, rays, ts, rgbs, u_cam, u_sun, epoch, step, torch.float32, u_retry)
    _, g64, o64 = reference(sd, rays, ts, rgbs, u_cam, u_sun, epoch, step, torch.float64, u_retry)
    assert abs(a.loss.item() - l32.item()) < 1e-5
    exactness(tag + " d_origins", d_origins, g32, g64)
    exactness(tag + " d_offsets", d_off if pre is None else d_off - pre, o32, o64)
    return a, d_origins, d_off


@pytest.mark.parametrize("tag", ["e0_rgb", "e0", "e3"])
def test_fp32_origin_gradient_matches_reference_autograd(tag):
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    check_against_reference(tag, sd, rays, ts, rgbs, u_cam, u_sun, 2.0 / 128, 128)


# Measured on MI355X over the noise seeds 52, 53, 54 (bf16 context, pipelined path, against the fp32 context of the same library):
#   seed   d_origins rel L2 / cosine     d_offsets rel L2 / cosine
#    52    1.4312e-01 / 0.989734         1.4581e-01 / 0.989364
#    53    1.3752e-01 / 0.990962         1.2384e-01 / 0.992856
#    54    1.4163e-01 / 0.989953         1.8190e-01 / 0.984121
# The project's pair for bf16 PARAMETER gradients (relative L2 < 6e-2, cosine > 0.998) is NOT met: the origin gradient runs through the
# encoder derivative 2^k cos(2^k x), k <= 9, which multiplies the bf16 rounding of dY_0 / dY_5 and of the weights by up to 512, and a
# per-image sum over ~30 rays does not average it out.  Asserted: 2 x the worst relative L2 and 1 - 2 (1 - worst cosine).
BF16_REL_ORIGINS, BF16_COS_ORIGINS = 1.4312e-01, 0.989734
BF16_REL_OFFSETS, BF16_COS_OFFSETS = 1.8190e-01, 0.984121


def _rel_cos(got, ref):
    got, ref = got.double().flatten().cpu(), ref.double().flatten().cpu()
    return ((got - ref).norm() / ref.norm()).item(), (torch.dot(got, ref) / (got.norm() * ref.norm())).item()


@pytest.mark.parametrize("seed", [52, 53, 54])
def test_bf16_origin_gradient_close_to_fp32(seed):
    """bf16 context (layer-pipelined path) against the fp32 context, full step (shadow pass + uncertainty loss), same batch, noise of
    the three seeds.  Measured on MI355X: the table above (DESIGN.md 5 carries the same numbers); 6e-2 / 0.998 is not met."""
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    if seed != 52:
        _, _, _, u_cam, u_sun = orc.synthetic_batch(R, N_IMG, seed=seed)
    flags, kind, _ = flags_of("e3")
    res = {}
    for prec in ("fp32", "bf16"):
        a = Abi(make_field(sd, N_IMG, prec), R).step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind)
        res[prec] = a.origin_grad()
    (rel_o, cos_o), (rel_q, cos_q) = _rel_cos(res["bf16"][0], res["fp32"][0]), _rel_cos(res["bf16"][1], res["fp32"][1])
    print(f"origin-grad bf16 vs fp32, noise seed {seed}: d_origins rel={rel_o:.4e} cos={cos_o:.6f} | d_offsets rel={rel_q:.4e} cos={cos_q:.6f}")
    assert rel_o <= 2 * BF16_REL_ORIGINS and cos_o >= 1 - 2 * (1 - BF16_COS_ORIGINS), (rel_o, cos_o)
    assert rel_q <= 2 * BF16_REL_OFFSETS and cos_q >= 1 - 2 * (1 - BF16_COS_OFFSETS), (rel_q, cos_q)


def _edge_batch(n, ns, seed):
    sd = base_case()[0]
    rays, ts, rgbs, u_cam, u_sun = orc.synthetic_batch(n, N_IMG, seed=seed, n_samples=ns)
    return sd, rays, ts, rgbs, u_cam, u_sun


def test_edges_empty_ray_and_empty_shadow_ray():
    """Ray 5 misses the cube: no camera samples, its d_origins row is exactly 0.  Ray 7 clips a corner of the cube right under its top
    face: one camera sample, and its shadow ray leaves the cube before its first sample."""
    sd, rays, ts, rgbs, u_cam, u_sun = _edge_batch(R, 128, 52)
    rays = rays.clone()
    rays[5, 0], rays[5, 3:6] = 1.5, torch.tensor([1.0, 0.0, 0.0])
    d = torch.tensor([0.7, 0.7, -0.1])
    rays[7, 0:3], rays[7, 3:6] = torch.tensor([0.99, 0.99, 0.9995]), d / d.norm()
    a, d_origins, _ = check_against_reference("e3:edges", sd, rays, ts, rgbs, u_cam, u_sun, 2.0 / 128, 128, u_retry=u_cam)
    out = a.out.cpu()
    assert out[5, 14] == 0 and out[7, 14] == 1 and out[7, 15] == 0          # the cases are what the docstring says
    assert torch.equal(d_origins[5].cpu(), torch.zeros(3))


@pytest.mark.parametrize("n,ns", [(193, 128), (1, 128), (96, 37)])
def test_edges_sizes(n, ns):
    """193 rays (no multiple of anything), one ray, and 37 samples per ray (the sampler's one-slot-per-lane instance)."""
    step = 2.0 / ns
    assert int(2 / step) == ns
    sd, rays, ts, rgbs, u_cam, u_sun = _edge_batch(n, ns, 400 + n + ns)
    a, _, _ = check_against_reference(f"e3:n{n}_ns{ns}", sd, rays, ts, rgbs, u_cam, u_sun, step, ns)
    total = int(a.out[:, 14].sum().item())
    print(f"camera samples of the batch: {total} (multiple of 32: {total % 32 == 0})")
    if (n, ns) == (193, 128):
        assert total % 32 != 0      # the sample total that is no multiple of the tile


def test_edges_one_image_accumulates_and_leaves_other_rows_alone():
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    ts = torch.full_like(ts, 4)
    pattern = (torch.arange(N_IMG * 3, dtype=torch.float32).reshape(N_IMG, 3) * 0.25 - 1.0).cuda()
    _, _, d_off = check_against_reference("e3:one_image", sd, rays, ts, rgbs, u_cam, u_sun, 2.0 / 128, 128, d_offsets=pattern.clone())
    keep = [j for j in range(N_IMG) if j != 4]
    assert_same_bits("one image", "other rows of d_offsets", d_off[keep], pattern[keep])
    assert not torch.equal(d_off[4], pattern[4])


FLAG_SETS = (0, 1, 2, 3, 8, 10, 4, 5, 4 | 16)


@pytest.mark.parametrize("deterministic", [True, False])
def test_does_not_disturb_the_step_and_is_reproducible(deterministic, monkeypatch):
    """With EONERF_DETERMINISTIC=1: outputs and d_flat of a step with the origin gradient taken are bit-identical to those of a step
    without it.  In both modes: two identical step + origin-gradient sequences give bit-identical d_origins / d_offsets, and
    eonerf_render_workspace_bytes is what it was before the first pose call on the context."""
    if deterministic:
        monkeypatch.setenv("EONERF_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("EONERF_DETERMINISTIC", raising=False)
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    flags, kind, _ = flags_of("e3")
    for prec in ("fp32", "bf16"):
        a = Abi(make_field(sd, N_IMG, prec), R)
        sizes = [a.ws_bytes(fl, n) for fl in FLAG_SETS for n in (1, R, 4096)]
        a.step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind)
        out0, d0 = a.out.clone(), a.d_flat.clone()
        a.step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind)
        g1 = a.origin_grad()
        out1, d1 = a.out.clone(), a.d_flat.clone()
        a.step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind)
        g2 = a.origin_grad()
        assert sizes == [a.ws_bytes(fl, n) for fl in FLAG_SETS for n in (1, R, 4096)]
        assert_same_bits(prec, "d_origins (run 2 vs run 1)", g2[0], g1[0])
        assert_same_bits(prec, "d_offsets (run 2 vs run 1)", g2[1], g1[1])
        assert torch.isfinite(g1[0]).all() and g1[1].abs().sum() > 0
        if deterministic:
            assert_same_bits(prec, "out", out1, out0)
            assert_same_bits(prec, "d_flat", d1, d0)
            assert_same_bits(prec, "d_flat (third step)", a.d_flat, d0)


def test_refusals_leave_the_outputs_untouched():
    from eonerf_code_amd import _lib
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    flags, kind, _ = flags_of("e3")
    a = Abi(make_field(sd, N_IMG, "fp32"), R)
    dev = a.flat.device
    a.rays, a.img, a.flags = rays.cuda().contiguous(), ts.reshape(-1).cuda().contiguous(), flags
    a.ws = torch.empty(a.ws_bytes(flags), dtype=torch.uint8, device=dev)
    d_origins = torch.full((R, 3), 7.0, device=dev)
    d_offsets = torch.full((N_IMG, 3), 9.0, device=dev)
    scratch = torch.empty(a.scratch_bytes(), dtype=torch.uint8, device=dev)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_origins == 7.0).all()) and bool((d_offsets == 9.0).all())

    assert a.origin_grad_rc(d_origins, d_offsets, scratch) == E_STATE and untouched()               # no backward yet
    a.step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind, ws=a.ws)
    assert a.origin_grad_rc(d_origins, d_offsets, scratch, n=R - 1) == E_STATE and untouched()      # another n_rays
    assert a.origin_grad_rc(d_origins, d_offsets, scratch, flags=_lib.F_TRAIN) == E_STATE and untouched()      # other flags
    assert a.origin_grad_rc(d_origins, d_offsets, scratch, flags=_lib.F_SHADOWS) == E_STATE and untouched()    # not a training call
    assert a.origin_grad_rc(d_origins, d_offsets, scratch, scratch_bytes=scratch.numel() - 1) == E_WORKSPACE and untouched()
    assert a.origin_grad_rc(None, None, scratch) == E_ARG
    assert a.origin_grad_rc(d_origins, d_offsets, scratch) == 0 and not untouched()                 # (the record is not used up by a refusal)
    d_origins.fill_(7.0), d_offsets.fill_(9.0)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(a.L.eonerf_presample(a.ctx, a.ptr(a.rays), a.ptr(a.img), a.ptr(a.z), R, flags, a.ptr(cnt), a.ptr(a.ws), a.ws.numel(), a.stream()))
    assert a.origin_grad_rc(d_origins, d_offsets, scratch) == E_STATE and untouched()               # eonerf_presample ran
    _lib.check(a.L.eonerf_presample_cancel(a.ctx))
    a.step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind, ws=a.ws)
    other = torch.empty(a.ws_bytes(_lib.F_SHADOWS), dtype=torch.uint8, device=dev)
    out = torch.empty(R, 21, device=dev)
    u = [t.cuda().contiguous() for t in (u_cam, u_sun)]
    _lib.check(a.L.eonerf_render_forward(a.ctx, a.ptr(a.flat), a.ptr(a.rays), a.ptr(a.img), a.ptr(a.z), a.ptr(u[0]), None, a.ptr(u[1]), R, _lib.F_SHADOWS,
                                         a.ptr(out), a.ptr(cnt), a.ptr(other), other.numel(), a.stream()))
    assert a.origin_grad_rc(d_origins, d_offsets, scratch) == E_STATE and untouched()               # another call in between
    h = Abi(make_field(sd, N_IMG, "fp16x3"), R)
    h.rays, h.img, h.flags, h.ws = a.rays, a.img, flags, a.ws
    assert h.origin_grad_rc(d_origins, d_offsets, scratch) == E_UNSUPPORTED and untouched()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_workspace_contract(prec):
    """Guards around the scratch and both outputs stay clean; the render workspace holds the same bits before and after the call."""
    sd, rays, ts, rgbs, u_cam, u_sun = base_case()
    flags, kind, _ = flags_of("e3")
    a = Abi(make_field(sd, N_IMG, prec), R).step(rays, ts, rgbs, (u_cam, None, u_sun), flags, kind)
    dev = a.flat.device
    bufs = [Guarded("scratch", a.scratch_bytes(), dev), Guarded("d_origins", R * 3 * 4, dev), Guarded("d_offsets", N_IMG * 3 * 4, dev, fill=0)]
    before = a.ws.clone()
    assert a.origin_grad_rc(bufs[1], bufs[2], bufs[0]) == 0
    torch.cuda.synchronize()
    check_guards("eonerf_render_origin_grad", bufs)
    assert_same_bits("eonerf_render_origin_grad", "render workspace", a.ws, before)
    want = a.origin_grad()
    assert_same_bits("guarded vs plain", "d_origins", bufs[1].view(torch.float32, R, 3), want[0])
    assert_same_bits("guarded vs plain", "d_offsets", bufs[2].view(torch.float32, N_IMG, 3), want[1])
