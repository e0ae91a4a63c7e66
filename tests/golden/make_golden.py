#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE's own Python code
(/root/reference, read-only) on CPU in the build container.  Never runs on the GPU box: only the
.npz outputs (data: inputs + expected outputs) are committed, no reference source travels.

Third-party packages that are absent here are replaced at import time by placeholder modules
that only supply the missing NAMES (no arithmetic): torchvision.transforms, rasterio, rpcm,
nerfacc.OccGridEstimator / nerfacc.rendering.  Groups G1..G7 therefore execute reference code only.

Group G8 additionally binds nerfacc.volrend's three functions to oracle/nerfacc_restated.py (the
published v0.5.2 algorithm restated; nerfacc itself is un-vendored, setup_env.sh:10) so that the
reference's EONerfMLP.rendering / compute_geometric_shadows / render_image run end to end.  G8 pins
everything in those functions EXCEPT the nerfacc arithmetic, which stays "parity unpinned".

Usage:  python tests/golden/make_golden.py        (writes tests/golden/g*.npz)
"""
import os
import sys
import types

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")      # the same MKL code path on every CPU, as tests/conftest.py sets it

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)          # must precede site-packages: a HuggingFace `datasets` package is installed

from oracle import nerfacc_restated as nv          # noqa: E402
from oracle import eonerf_oracle as orc            # noqa: E402  (only for closed_form_state_dict / synthetic rays)


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Missing:
    def __init__(self, *a, **k):
        raise RuntimeError("placeholder for an un-vendored third-party symbol was called")


_placeholder("torchvision", transforms=_placeholder("torchvision.transforms"))
_placeholder("rasterio")
_placeholder("rpcm", RPCModel=_Missing)
_placeholder("nerfacc", OccGridEstimator=_Missing, rendering=_Missing,
             render_transmittance_from_density=nv.render_transmittance_from_density,
             accumulate_along_rays=nv.accumulate_along_rays)
_placeholder("nerfacc.volrend", render_weight_from_density=nv.render_weight_from_density,
             accumulate_along_rays=nv.accumulate_along_rays,
             render_transmittance_from_density=nv.render_transmittance_from_density)

from radiance_fields.mlp import SinusoidalEncoder, MLP, DenseLayer      # noqa: E402
from radiance_fields import eonerf as ref_eonerf                         # noqa: E402
import sat_rendering as ref_sr                                           # noqa: E402
import metrics as ref_metrics                                            # noqa: E402
from datasets.satellite import define_satrays_from_tensors              # noqa: E402

torch.set_num_threads(4)


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"wrote {name}.npz", {k: tuple(v.shape) for k, v in out.items()})


GRAD_STRIDE = 61


def compact_grad(g):
    """Large gradient tensors are committed as [sum, sum|.|, every GRAD_STRIDE-th element] to keep fixtures small."""
    flat = g.detach().reshape(-1).double()
    head = torch.stack([flat.sum(), flat.abs().sum()])
    body = flat if flat.numel() <= 1024 else flat[::GRAD_STRIDE]
    return torch.cat([head, body])


def rand_with_replay(shape, seed):
    """Return u = torch.rand(shape) and leave the global generator in the state where the NEXT
    rand_like(shape) reproduces exactly u (how the reference's perturb_z_vals noise is captured)."""
    torch.manual_seed(seed)
    u = torch.rand(shape)
    torch.manual_seed(seed)
    return u


# ------------------------------------------------------------------ G1 encoder
def g1():
    x = torch.tensor([[0.0, 0.0, 0.0], [1.0, -1.0, 1.0], [1e-3, -1e-3, 0.5], [0.999999, -0.999999, 0.25],
                      [0.3, 0.7, -0.9], [-0.123456, 0.654321, 0.98]], dtype=torch.float32)
    g = torch.Generator().manual_seed(1)
    x = torch.cat([x, torch.rand(58, 3, generator=g) * 2 - 1], 0)
    save("g1_encoder", x=x, enc10=SinusoidalEncoder(3, 0, 10, True)(x.clone()),
         enc4=SinusoidalEncoder(3, 0, 4, True)(x.clone()))


def _fill(t, c):
    idx = torch.arange(t.numel(), dtype=torch.float64).reshape(t.shape)
    return (0.5 * torch.sin(0.37 * idx + c)).float()


# ------------------------------------------------------------------ G2 MLP skip-concat
def g2():
    m = MLP(input_dim=7, output_dim=3, net_depth=6, net_width=16, skip_layer=4)
    d = DenseLayer(16, 5)
    with torch.no_grad():
        for c, p in enumerate(list(m.parameters()) + list(d.parameters())):
            p.copy_(_fill(p, c))
    g = torch.Generator().manual_seed(2)
    x = torch.rand(33, 7, generator=g) * 2 - 1
    h = torch.rand(33, 16, generator=g) * 2 - 1
    sd = {f"mlp.{k}": v for k, v in m.state_dict().items()}
    sd.update({f"dense.{k}": v for k, v in d.state_dict().items()})
    save("g2_mlp", x=x, h=h, y_mlp=m(x), y_dense=d(h), **sd)


# ------------------------------------------------------------------ G3/G7 field forward + grads
def _ref_field(n_img, sd):
    f = ref_eonerf.EONerfMLP(n_img, radiometric_normalization=True)
    missing = f.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return f


def g3_g7():
    n_img = 5
    sd = orc.closed_form_state_dict(n_img)
    f = _ref_field(n_img, sd)
    manifest = {k: (tuple(v.shape), str(v.dtype)) for k, v in f.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    x = torch.rand(512, 3, generator=g) * 2 - 1
    sun = torch.randn(512, 3, generator=g)
    sun = sun / sun.norm(dim=1, keepdim=True)
    img = torch.randint(0, n_img, (512, 1), generator=g)
    with torch.no_grad():
        sigma, albedo, ambient, ts, tb = f(x, sun, img)
        dens = f.query_density(x)
        opac = f.query_opacity(x, 2.0 / 128)
    save("g3_field_w256", x=x, sun=sun, img=img, sigma=sigma, albedo=albedo, ambient=ambient, ts=ts, tb=tb,
         density=dens, opacity=opac, n_img=n_img,
         manifest_keys=np.array(list(manifest.keys())),
         manifest_shapes=np.array([str(v[0]) for v in manifest.values()]),
         manifest_dtypes=np.array([v[1] for v in manifest.values()]))

    # G7: autograd gradients w.r.t. weights AND input positions on 64 points
    xs = x[:64].clone().requires_grad_(True)
    f.zero_grad()
    sigma, albedo, ambient, ts, tb = f(xs, sun[:64], img[:64])
    cw = torch.linspace(0.5, 1.5, 64)[:, None]
    scalar = (cw * sigma).sum() + (albedo * cw).sum() * 0.7 + ambient.sum() * 0.3 + (ts * cw).sum() * 1.1 + tb.sum() * 0.9
    scalar.backward()
    grads = {("grad." + k): compact_grad(p.grad) for k, p in f.named_parameters() if p.grad is not None}
    xd = x[:64].clone().requires_grad_(True)
    (f.query_density(xd) * cw).sum().backward()
    save("g7_field_grads", scalar=scalar, dx=xs.grad, dx_density=xd.grad, **grads)

    # reduced width, reference-constructed seed-42 init, committed in full
    torch.manual_seed(42)
    f64 = ref_eonerf.EONerfMLP(3, net_width=64, radiometric_normalization=True)
    with torch.no_grad():
        s2, a2, am2, ts2, tb2 = f64(x[:128], sun[:128], img[:128] % 3)
        d2 = f64.query_density(x[:128])
    save("g3_field_w64", x=x[:128], sun=sun[:128], img=img[:128] % 3, sigma=s2, albedo=a2, ambient=am2, ts=ts2, tb=tb2,
         density=d2, **{"sd." + k: v for k, v in f64.state_dict().items()})


# ------------------------------------------------------------------ G4 sampler
def _g4_rays():
    rays, ts, _, _, _ = orc.synthetic_batch(60, 5, seed=4)
    o, d = rays[:, :3].clone(), rays[:, 3:6].clone()
    o[50:55, :2] = torch.tensor([[0.97, 0.0], [-0.97, 0.5], [0.0, 0.99], [0.9, 0.9], [-0.95, -0.95]])
    d[50:55] = torch.tensor([[0.6, 0.0, -0.8], [-0.6, 0.0, -0.8], [0.0, 0.8, -0.6], [0.5, 0.5, -0.7071], [-0.7, -0.7, -0.14]])
    d = d / d.norm(dim=1, keepdim=True)
    extra_o = torch.tensor([[1.5, 0.0, 0.5], [0.0, 0.0, 1.0], [0.2, 0.3, 0.9999], [0.0, 0.0, 0.0]])
    extra_d = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])
    return torch.cat([o, extra_o]), torch.cat([d, extra_d])   # ray 60: no valid sample; 61: starts on the face; 62: leaves at once


def g4():
    o, d = _g4_rays()
    step = 2.0 / 128
    u = rand_with_replay((o.shape[0], 128), 44)
    ri, ts_, te_ = ref_sr.satnerf_sampling(o, d, {"render_step_size": step}, near=torch.zeros(o.shape[0], 1))
    rays_nt = types.SimpleNamespace(origins=o)
    pts = ref_sr.count_number_of_pts_per_nerfacc_ray(rays_nt, ri)
    z = torch.linspace(0, 1, 128)[None].repeat(4, 1) * 2
    u4 = rand_with_replay((4, 128), 45)
    zp = ref_sr.perturb_z_vals(z, True)
    save("g4_sampling", origins=o, viewdirs=d, u=u, step=step, ray_indices=ri, t_starts=ts_, t_ends=te_,
         pts_per_ray=pts, z_in=z, u4=u4, z_perturbed=zp, z_steps=torch.linspace(0, 1, 128))


# ------------------------------------------------------------------ G5 dense compositing cross-check
def g5():
    g = torch.Generator().manual_seed(5)
    z = torch.sort(torch.rand(16, 128, generator=g) * 2, dim=1).values
    sig = torch.rand(16, 128, generator=g) * 8
    sig[3] = 0.0
    sig[4, 50:] = 500.0
    w, t, a = ref_eonerf.weights_from_sigma(z, sig)
    save("g5_weights_from_sigma", z=z, sigma=sig, weights=w, trans=t, alphas=a)


# ------------------------------------------------------------------ G6 metrics
def g6():
    g = torch.Generator().manual_seed(6)
    gt, pred = torch.rand(40, 3, generator=g), torch.rand(40, 3, generator=g)
    beta = torch.rand(40, 1, generator=g) + 0.05
    loss, ld = ref_metrics.uncertainty_aware_loss(gt, pred, beta)
    gd = torch.rand(40, generator=g) * 2 - 0.3
    pd = torch.rand(40, generator=g) * 2
    conf = torch.randint(0, 8, (40,), generator=g).float()
    dl, _ = ref_metrics.depth_loss_L2(gd, pd, conf, 100)
    dl_noconf, _ = ref_metrics.depth_loss_L2(gd, pd, None, 100)
    sm = (torch.rand(40, generator=g) > 0.4).float()
    gs = torch.rand(40, generator=g)
    sl, _ = ref_metrics.shadow_loss_L2(sm, gs)
    save("g6_metrics", gt=gt, pred=pred, beta=beta, unc_loss=loss, unc_color=ld["coarse_color"], unc_logbeta=ld["coarse_logbeta"],
         gt_depth=gd, pred_depth=pd, conf=conf, depth_loss=dl, depth_loss_noconf=dl_noconf, smask=sm, geo=gs, shadow_loss=sl,
         psnr=ref_metrics.psnr(pred, gt), mse=ref_metrics.mse(pred, gt),
         mse_torch=torch.nn.functional.mse_loss(pred, gt))


# ------------------------------------------------------------------ G8 end-to-end (reference code + restated nerfacc)
def g8():
    n_img, R = 5, 48
    step = 2.0 / 128
    sd = orc.closed_form_state_dict(n_img)
    # make density matter: scale the sigma head so rays terminate inside the cube
    sd["sigma_layer.output_layer.bias"] = sd["sigma_layer.output_layer.bias"] + 1.5
    f = _ref_field(n_img, sd)
    rays, ts, rgbs, _, _ = orc.synthetic_batch(R, n_img, seed=8)
    o, d = _g4_rays()
    rays[40:44, :3], rays[40:44, 3:6] = o[50:54], d[50:54]        # rays that exit through the side faces
    satrays = define_satrays_from_tensors(rays, ts)
    args = types.SimpleNamespace()
    out = {"rays": rays, "ts": ts, "rgbs": rgbs, "step": step, "n_img": n_img, "sigma_bias_shift": 1.5}

    rays[42, 1] = 0.95                                            # keep every ray non-empty in the main cases
    satrays = define_satrays_from_tensors(rays, ts)
    out["rays"] = rays
    rays_retry = rays.clone()
    rays_retry[42, 1] = 0.99                                      # ray 42 gets 0 samples -> "resample" branch (:260-262)
    out["rays_retry"] = rays_retry

    cases = (("e0", 0, False, satrays), ("e3", 3, False, satrays), ("e3eval", 3, True, satrays),
             ("e3retry", 3, False, define_satrays_from_tensors(rays_retry, ts)))
    for tag, epoch, ev, sr in cases:
        seed = 800 + len(tag) * 7 + epoch + int(ev)
        torch.manual_seed(seed)
        u1, u2, u3 = torch.rand(R, 128), torch.rand(R, 128), torch.rand(R, 128)
        torch.manual_seed(seed)          # rand_like draws: camera pass, [retry camera pass], then sun pass
        f.zero_grad()
        res, n = ref_sr.render_image(f, None, sr, None, args, epoch_idx=epoch, chunk=R,
                                     render_step_size=step, eval=ev)
        keys = ["rgb", "depth", "albedo_rgb", "ambient_rgb", "geo_shadows", "transient_s", "beta", "entropy",
                "pts_per_ray", "sc_pts_per_ray", "opacity_after_surface", "shadowless_rgb"]
        packed = torch.cat([res[k] for k in keys], dim=1)
        retried = bool((packed[:, 14] == 0).any())
        assert retried == (tag == "e3retry")
        out.update({f"{tag}.u_cam": u1, f"{tag}.u_retry": u2 if retried else torch.zeros(0),
                    f"{tag}.u_sun": u3 if retried else u2, f"{tag}.out": packed, f"{tag}.n_samples": n})
        if not ev:   # training gradients through the whole path (train_eonerf.py:139-143,160)
            if epoch < 2:
                loss = torch.nn.functional.mse_loss(res["rgb"], rgbs)
            else:
                loss, _ = ref_metrics.uncertainty_aware_loss(rgbs, res["rgb"], res["beta"])
            loss.backward()
            out[f"{tag}.loss"] = loss
            if tag != "e3retry":
                for k, p in f.named_parameters():
                    out[f"{tag}.grad.{k}"] = compact_grad(p.grad if p.grad is not None else torch.zeros_like(p))

    # only_depth branch (sat_rendering.py:227-249)
    torch.manual_seed(900)
    u_cam = torch.rand(R, 128)
    torch.manual_seed(900)
    with torch.no_grad():
        res, n = ref_sr.render_image(f, None, satrays, None, args, epoch_idx=3, chunk=R, render_step_size=step, only_depth=True)
    out.update({"od.u_cam": u_cam, "od.depth": res["depth"], "od.n_samples": n})

    # chunked call == concatenation of chunks, each drawing its own noise (sat_rendering.py:252)
    torch.manual_seed(901)
    u_chunks = [(torch.rand(16, 128), torch.rand(16, 128)) for _ in range(3)]
    torch.manual_seed(901)
    with torch.no_grad():
        res, n = ref_sr.render_image(f, None, satrays, None, args, epoch_idx=3, chunk=16, render_step_size=step)
    out.update({"ch.u_cam": torch.cat([a for a, _ in u_chunks]), "ch.u_sun": torch.cat([b for _, b in u_chunks]),
                "ch.rgb": res["rgb"], "ch.depth": res["depth"], "ch.geo": res["geo_shadows"], "ch.n_samples": n})
    save("g8_render", **out)


# ------------------------------------------------------------------ G10 other step sizes: n_samples = int(2 / render_step_size) = 64, 256
def g10(ns):
    """sat_rendering.py:64 / opt.py:54 accept any --n_samples; the build implements every size up to 256 (round 6; 64 / 128 / 256 before).  The G4 sampler rays and a short G8
    (render_image forward for epoch_idx 0 and 3, loss, reference autograd) at the other two sizes."""
    step = 2.0 / ns
    o, d = _g4_rays()
    u = rand_with_replay((o.shape[0], ns), 44 + ns)
    ri, ts_, te_ = ref_sr.satnerf_sampling(o, d, {"render_step_size": step}, near=torch.zeros(o.shape[0], 1))
    pts = ref_sr.count_number_of_pts_per_nerfacc_ray(types.SimpleNamespace(origins=o), ri)
    out = {"origins": o, "viewdirs": d, "u": u, "step": step, "ray_indices": ri, "t_starts": ts_, "t_ends": te_, "pts_per_ray": pts,
           "z_steps": torch.linspace(0, 1, ns)}
    n_img, R = 5, 32
    sd = orc.closed_form_state_dict(n_img)
    sd["sigma_layer.output_layer.bias"] = sd["sigma_layer.output_layer.bias"] + 1.5
    f = _ref_field(n_img, sd)
    rays, ts, rgbs, _, _ = orc.synthetic_batch(R, n_img, seed=8 + ns)
    rays[28:31, :3], rays[28:31, 3:6] = o[50:53], d[50:53]        # rays that exit through the side faces ...
    rays[28:31, :2] *= 0.93                                       # ... after a few samples at every step size (no empty ray: no retry draw)
    satrays = define_satrays_from_tensors(rays, ts)
    args = types.SimpleNamespace()
    out.update({"rays": rays, "ts": ts, "rgbs": rgbs, "n_img": n_img, "sigma_bias_shift": 1.5})
    for tag, epoch in (("e0", 0), ("e3", 3)):
        seed = 1000 + ns + epoch
        torch.manual_seed(seed)
        u1, u2 = torch.rand(R, ns), torch.rand(R, ns)
        torch.manual_seed(seed)          # rand_like draws: camera pass, then sun pass
        f.zero_grad()
        res, n = ref_sr.render_image(f, None, satrays, None, args, epoch_idx=epoch, chunk=R, render_step_size=step)
        keys = ["rgb", "depth", "albedo_rgb", "ambient_rgb", "geo_shadows", "transient_s", "beta", "entropy",
                "pts_per_ray", "sc_pts_per_ray", "opacity_after_surface", "shadowless_rgb"]
        packed = torch.cat([res[k] for k in keys], dim=1)
        assert not (packed[:, 14] == 0).any()      # no retry draw in this fixture
        out.update({f"{tag}.u_cam": u1, f"{tag}.u_sun": u2, f"{tag}.out": packed, f"{tag}.n_samples": n})
        if epoch < 2:
            loss = torch.nn.functional.mse_loss(res["rgb"], rgbs)
        else:
            loss, _ = ref_metrics.uncertainty_aware_loss(rgbs, res["rgb"], res["beta"])
        loss.backward()
        out[f"{tag}.loss"] = loss
        for k, p in f.named_parameters():
            out[f"{tag}.grad.{k}"] = compact_grad(p.grad if p.grad is not None else torch.zeros_like(p))
    save(f"g10_n{ns}", **out)


# ------------------------------------------------------------------ G9 vanilla NeRF field (BASELINE.json configs[0])
def vanilla_fill(name, shape):
    """Closed-form weights of the G9 field: only this formula is committed, both sides regenerate the tensors from it."""
    c = sum(ord(ch) for ch in name) % 17
    n = 1
    for d in shape:
        n *= d
    idx = torch.arange(n, dtype=torch.float64).reshape(shape)
    fan = shape[-1] + shape[0] if len(shape) == 2 else 1
    scale = (6.0 / fan) ** 0.5 if len(shape) == 2 else 0.01
    return (scale * torch.sin(0.37 * idx + c)).float()


def vanilla_inputs(n_rays=256, n_samples=64):
    """configs[0]: 256 rays x 64 samples.  Positions [R,S,3] inside the unit cube, one view direction per ray [R,3]."""
    r = torch.arange(n_rays, dtype=torch.float64)[:, None]
    k = torch.arange(n_samples, dtype=torch.float64)[None, :]
    x = torch.stack([torch.sin(0.11 * r + 0.07 * k), torch.cos(0.05 * r - 0.13 * k), torch.sin(0.017 * r * k + 0.3)], dim=-1).float() * 0.95
    d = torch.stack([torch.sin(0.3 * r[:, 0]), torch.cos(0.2 * r[:, 0]), -torch.ones(n_rays, dtype=torch.float64)], dim=-1)
    d = (d / d.norm(dim=-1, keepdim=True)).float()
    return x, d


def g9():
    from radiance_fields.mlp import VanillaNeRFRadianceField
    f = VanillaNeRFRadianceField()                                  # the shipped geometry: 8 x 256, skip 4, condition head 1 x 128
    with torch.no_grad():
        for name, p in f.named_parameters():
            p.copy_(vanilla_fill(name, tuple(p.shape)))
    x, d = vanilla_inputs()
    R, S = x.shape[:2]
    # flattened samples, as the reference's renderers hand them to a field (SinusoidalEncoder.forward tiles its mask for 2-D input
    # only, mlp.py:207); the view direction of a ray is repeated for its samples
    x = x.reshape(R * S, 3)
    d = d[:, None, :].expand(R, S, 3).reshape(R * S, 3)
    xg = x.clone().requires_grad_(True)
    rgb, sigma = f(xg, d)
    dens = f.query_density(x)
    opac = f.query_opacity(x, 2.0 / 64)
    # a plumbing train step's loss and gradients (train_mlp_nerf.py renders rgb/opacity from these and back-propagates an L1-type loss)
    cw = torch.linspace(0.5, 1.5, 3)[None, :]
    loss = (rgb * cw).sum() / rgb.numel() + 0.1 * sigma.sum() / sigma.numel()
    loss.backward()
    grads = {f"grad.{n}": compact_grad(p.grad) for n, p in f.named_parameters()}
    manifest = np.array([f"{k}:{tuple(v.shape)}:{str(v.dtype).replace('torch.', '')}" for k, v in f.state_dict().items()])
    save("g9_vanilla", rgb=rgb[::4], sigma=sigma[::4], density=dens[::4], opacity=opac[::4], loss=loss, dx=xg.grad[::8],
         n_rays=R, n_samples=S, manifest=manifest, **grads)


if __name__ == "__main__":
    only = sys.argv[1:]
    for name, fn in (("g1", g1), ("g2", g2), ("g3_g7", g3_g7), ("g4", g4), ("g5", g5), ("g6", g6), ("g8", g8), ("g9", g9),
                     ("g10", lambda: (g10(64), g10(256))), ("g10b", lambda: (g10(96), g10(192)))):      # g10b (round 6): step sizes that are not a power of two
        if not only or name in only:
            fn()
