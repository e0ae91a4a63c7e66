"""A/B of the surface normals (include/eonerf_normals.h; normals.render_normals) on one GPU, by the protocol of scripts/quantile_ab.py.
The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- rendered on the fp16x3 export context: one
512 x 512 nadir view (262,144 rays, chunk 5120) at 128 samples per ray.
Two measurements.
  render    render_normals against render_image(only_depth=True) on the same rays, the parent's code unchanged; the two alternate, three
            rounds after a warm-up of both, device events around work that ends in one synchronise; the baseline's own max - min is
            printed beside the ratio.  The chain carries four columns per sample instead of one: a ratio near 4 is the expectation.
  gradient  for the sample positions of one chunk: normals.density_gradient on the export context against the existing route,
            query_density under autograd (eonerf_field_forward_train + eonerf_field_backward) on an fp32 training context.
    python3 scripts/normals_ab.py [--out profiles/normals_ab.txt] [--side 512] [--rounds 3] [--steps 2000]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import STEP, Z_SCALE, twin_train
from eonerf_code_amd import dsm
from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
from eonerf_code_amd.normals import density_gradient, render_normals, slope_aspect
from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
from eonerf_code_amd.sat_rendering import render_image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
args = ap.parse_args()

CHUNK, NS, KEY = 5120, 128, 7
SC, SUN = [250.0, 250.0, Z_SCALE], (35.0, 160.0)
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
rays = dsm.nadir_rays(args.side, args.side, SC, *SUN, device=dev)
sat = define_satrays_from_tensors(rays, torch.zeros(rays.shape[0], 1, dtype=torch.int64, device=dev))
n_rays = rays.shape[0]


def baseline():
    field.set_noise_seed(KEY)
    return render_image(field, None, sat, None, None, chunk=CHUNK, render_step_size=STEP, only_depth=True, eval=True)


def normals_leg():
    field.set_noise_seed(KEY)
    return render_normals(field, None, sat, chunk=CHUNK, render_step_size=STEP, scene_scale=SC)


def timed(fn, grad=False):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with torch.set_grad_enabled(grad):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def line(tag, b, g, what):
    (bm, bs), (gm, gs) = stats(b), stats(g)
    return (f"{tag}: baseline {' '.join(f'{v:8.2f}' for v in b)} (median {bm:.2f}, max - min {bs:.2f}) | {what} {' '.join(f'{v:8.2f}' for v in g)} "
            f"(median {gm:.2f}, max - min {gs:.2f}) | ratio {gm / bm:.3f}")


lines = [f"surface normals A/B: {args.side} x {args.side} nadir view ({n_rays} rays, chunk {CHUNK}), {NS} samples per ray; twin_train bf16 field, {args.steps} steps",
         f"alternating, {args.rounds} rounds after a warm-up of both; ms, device events around work ending in one synchronise"]
(_, (b_res, b_n)), (_, (q_res, q_n)) = timed(baseline), timed(normals_leg)      # warm-up of both
lines.append(f"export context after the warm-up: {field.eval_precision}" + ("" if field.eval_precision == "fp16x3" else
             " (a derivative column left fp16's range: both legs below run on the fp32 context)"))
assert torch.equal(b_res["depth"], q_res["depth"]) and b_n == q_n       # the expected depth is the baseline's, bit for bit
b, g = [], []
for _ in range(args.rounds):
    b.append(timed(baseline)[0])
    g.append(timed(normals_leg)[0])
lines.append(line(f"render ({b_n} samples)", b, g, "render_normals"))
print(lines[-1], flush=True)
slope, _ = slope_aspect(q_res["normal"])
hit = q_res["acc"].reshape(-1) > 0.5
agree = (torch.linalg.vector_norm(q_res["normal_raw"], dim=1) / q_res["acc"].reshape(-1))[hit]
lines.append(f"the view: slope median {slope[hit].median().item():.2f} deg, p99 {slope[hit].quantile(0.99).item():.2f} deg; |N| / A median {agree.median().item():.3f}, "
             f"p1 {agree.quantile(0.01).item():.3f}")

# the existing route on the same positions: the samples of the first chunk
first = define_satrays_from_tensors(rays[:CHUNK], torch.zeros(CHUNK, 1, dtype=torch.int64, device=dev))
field.set_noise_seed(KEY)
res, _ = render_normals(field, None, first, chunk=CHUNK, render_step_size=STEP, return_samples=True)
ri, t0, t1, _, _ = res["samples"]
pos = (rays[ri, 0:3] + rays[ri, 3:6] * ((t0 + t1) / 2)[:, None]).contiguous()
f32 = EONerfMLP(field.n_input_images, radiometric_normalization=field.radiometric_normalization, precision="fp32").to(dev)
f32.load_state_dict(field.state_dict())
f32.train()


def autograd_route():
    x = pos.clone().requires_grad_(True)
    sigma = f32.query_density(x)
    return torch.autograd.grad(sigma.sum(), x)[0]


def forward_mode():
    return density_gradient(field, pos)[1]


(_, g_auto), (_, g_fwd) = timed(autograd_route, True), timed(forward_mode)
rel = (torch.linalg.vector_norm(g_fwd - g_auto) / torch.linalg.vector_norm(g_auto)).item()
b, g = [], []
for _ in range(args.rounds):
    b.append(timed(autograd_route, True)[0])
    g.append(timed(forward_mode)[0])
lines.append(line(f"gradient at {pos.shape[0]} sample positions (baseline: query_density autograd, fp32 training context)", b, g, f"density_gradient ({field.eval_precision})"))
lines.append(f"relative L2 between the two gradients: {rel:.2e}; {pos.shape[0] / stats(g)[0] / 1e3:.2f} M points/s forward mode, {pos.shape[0] / stats(b)[0] / 1e3:.2f} M points/s autograd")
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
