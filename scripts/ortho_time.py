"""Device time of the true orthophoto (include/eonerf_ortho.h, eonerf_code_amd/ortho.py) on one GPU: synthetic RPCs and random images,
a 512 x 512 nadir grid (262,144 points), K = 20 images of 1024 x 1024 x 3, on a random-init field.  A record, not a criterion: the
parent commit has nothing to compare it with.  Four figures, each the median of `--rounds` repeats after a warm-up, device events
around work that ends in one synchronise; each repeat loops the call often enough to fill a window of tens of milliseconds.
  ground   eonerf_ortho_ground on the 262,144 points
  gather   eonerf_ortho_gather, all 20 images (per image beside it)
  fuse     eonerf_ortho_fuse, mean and median, K = 20
  whole    one orthorectify call: the sun sweep (one camera pass, 20 shadow passes at 128 samples, chunk 5120) plus the three above
With a random-init field the depth is no surface and the occlusion test rejects little or nothing: the sweep's time is that of the
dense render, the gather's that of a fully visible scene (its worst case).  The occlusion test through a converged field is not measured.
    python3 scripts/ortho_time.py [--out profiles/ortho_time.txt] [--side 512] [--images 20] [--rounds 5]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

from eonerf_code_amd import dsm, ortho
from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
from oracle import raygen_oracle as RO

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--images", type=int, default=20)
ap.add_argument("--image_side", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()

assert torch.cuda.is_available(), "ortho_time.py measures on the GPU; there is no fall-back"
dev = torch.device("cuda", 0)
K, SIDE, IMG, C = args.images, args.side, args.image_side, 3
LAT0, LON0 = 30.33, -81.66
zone, south = RO.utm_zone_number(LAT0, LON0), False
e0, n0 = RO.utm_forward(np.array([LAT0]), np.array([LON0]), zone, south)
OFF, SC = [round(float(e0[0])), round(float(n0[0])), 20.0], [300.0, 300.0, 60.0]
MIN_ALT, MAX_ALT = -10.0, 50.0
rpcs = [RO.rescale_rpc(RO.synthetic_rpc(100 + k, lat0=LAT0, lon0=LON0), IMG / 2048.0) for k in range(K)]
g = torch.Generator(device=dev).manual_seed(3)
images = [torch.rand(IMG, IMG, C, generator=g, device=dev) for _ in range(K)]
torch.manual_seed(5)
field = EONerfMLP(K, radiometric_normalization=True).to(dev).eval()
rays = dsm.nadir_rays(SIDE, SIDE, SC, 0.0, 0.0, device=dev)
n = rays.shape[0]


def timed(fn, loops):
    e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0_.record()
    for _ in range(loops):
        out = fn()
    e1_.record()
    torch.cuda.synchronize()
    return e0_.elapsed_time(e1_) / loops, out


def measure(fn, loops):
    timed(fn, 1)                                                    # warm-up: code objects, allocator
    v = sorted(timed(fn, loops)[0] for _ in range(args.rounds))
    return v[len(v) // 2], v[-1] - v[0]


whole = lambda: ortho.orthorectify(field, images, rpcs, OFF, SC, zone, south, SIDE, SIDE, MIN_ALT, MAX_ALT, rays=rays, return_all=True)   # noqa: E731
_, first = timed(whole, 1)
depth, vis, lla, layers, weights = first["depth"], first["visibility"], first["lonlatalt"], first["layers"], first["weights"]
from eonerf_code_amd.datasets.satellite import _rpc_struct
structs = [_rpc_struct(r) for r in rpcs]
one, zero = [1.0] * C, [0.0] * C
lay, wgt = torch.empty_like(layers), torch.empty_like(weights)


def gather_all():
    for k in range(K):
        ortho._gather(lla, structs[k], images[k], one, zero, vis[k], 0.2, lay[k], wgt[k], None)


lines = [f"true orthophoto: {SIDE} x {SIDE} nadir grid ({n} points), K = {K} images of {IMG} x {IMG} x {C}, synthetic RPCs, random-init field "
         f"({field.eval_precision} export context, 128 samples per ray, chunk 5120); ms, median of {args.rounds} (max - min), device events",
         f"cells seen by at least one image: {int((first['count'] > 0).sum())} of {n}; mean images per cell {float(first['count'].float().mean()):.2f}"]
for tag, fn, loops in (("eonerf_ortho_ground", lambda: ortho.ground_points(rays, depth, OFF, SC, zone, south), 50),
                       (f"eonerf_ortho_gather x {K}", gather_all, 5),
                       ("eonerf_ortho_fuse mean", lambda: ortho.fuse_layers(layers, weights, "mean"), 50),
                       ("eonerf_ortho_fuse median", lambda: ortho.fuse_layers(layers, weights, "median"), 50),
                       ("orthorectify (sweep + ground + gather + fuse)", whole, 1)):
    m, s = measure(fn, loops)
    extra = f"  = {m / K:.3f} per image" if tag.startswith("eonerf_ortho_gather") else ""
    lines.append(f"  {tag:48s} {m:10.3f} ({s:.3f}){extra}")
    print(lines[-1], flush=True)
lines.append("not measured: the occlusion test through a converged field (no such checkpoint exists); a random-init field's depth is no surface")
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
