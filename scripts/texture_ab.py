"""Texture baking (eonerf_code_amd/csrc/eonerf_texture.h; eonerf_code_amd/texture.py) on one GPU, by the protocol of scripts/raycast_ab.py.
The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- meshed on a --res^3 lattice (256) and simplified on
cells of --simplify lattice spacings (2), placed on the ground by tests/ortho_restated.scene_frame; K synthetic images (the field's image
count) of --side px (512) with the RPCs of oracle.raygen_oracle.synthetic_rpc; --texels texels a leg (4).
  * the three stages of bake_texture over the whole atlas in chunks of --chunk texels, timed apart: eonerf_texture_samples, the K any-hit
    casts of MeshRaycaster.occluded per chunk, eonerf_texture_bake (the product's form: normals, angle weight, median);
  * the baseline for the bake -- the path that existed before: K eonerf_ortho_gather calls and one eonerf_ortho_fuse on the same points and
    the same occlusion (visibility 1 - blocked), chunked alike -- against eonerf_texture_bake with normal = NULL, the form that equals it bit
    for bit (tests/test_texture_gpu.py), and the peak device memory of both above the tables they share;
  * mesh/textured of the product's result.
The legs alternate, --rounds rounds (5) after a warm-up of all; device events around work that ends in one synchronise; max - min beside
the median.  A 2,000-step field is not a converged scene: the figures show the tool.
    python3 scripts/texture_ab.py [--out profiles/texture_ab.txt] [--rounds 5] [--steps 2000] [--res 256] [--simplify 2] [--texels 4]"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import ortho_restated as OR
from bf16_common import twin_train
from eonerf_code_amd import _lib
from eonerf_code_amd._lib import _ptr, _stream
from eonerf_code_amd.datasets.satellite import _rpc_struct
from eonerf_code_amd.mesh import MeshRaycaster, extract_mesh, level_from_opacity
from eonerf_code_amd.ortho import _f3
from eonerf_code_amd.texture import _bake, _tables, _view_tables, atlas_layout, bake_texture
from oracle import raygen_oracle as RO

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--simplify", type=int, default=2)
ap.add_argument("--texels", type=int, default=4)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--chunk", type=int, default=1 << 20)
args = ap.parse_args()

dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
L = _lib.lib()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with torch.no_grad():
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def row(tag, v, extra=""):
    m, s = stats(v)
    return f"  {tag:<52}{' '.join(f'{t:9.3f}' for t in v)}   median {m:9.3f} ms, max - min {s:.3f}{extra}"


def finish(lines):
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


level = level_from_opacity(0.5, 2.0 / 128)
mesh = extract_mesh(field, resolution=args.res, level=level, simplify=args.simplify, normals=False, albedo=False)
for a in range(9, 0, -1):                                 # a young field may not reach the default level: the densest level that has a surface
    if mesh["faces"].shape[0]:
        break
    level = level_from_opacity(a / 10, 2.0 / 128)
    mesh = extract_mesh(field, resolution=args.res, level=level, simplify=args.simplify, normals=False, albedo=False)
vertices, faces = mesh["vertices"].float().contiguous(), mesh["faces"].to(torch.int32).contiguous()
n_v, n_f = vertices.shape[0], faces.shape[0]
K, ch, T = int(field.n_input_images), 3, args.texels
zone, south, offset = OR.scene_frame(30.33)
scale = np.array(OR.SCENE_SCALE, dtype=np.float32)
rng = np.random.default_rng(11)
rpcs = [RO.rescale_rpc(RO.synthetic_rpc(70 + k, lat0=30.33, lon0=OR.LON0), args.side / 2048.0) for k in range(K)]
images = [torch.from_numpy(rng.uniform(0, 1, (args.side, args.side, ch)).astype(np.float32)).to(dev) for _ in range(K)]
min_alt, max_alt = -50.0, 90.0

lines = [f"texture baking: twin_train bf16 field, {args.steps} steps; {args.res}^3 lattice at level {level:.4f}, simplify={args.simplify}: {n_v} vertices, {n_f} faces; "
         f"{K} images of {args.side} x {args.side} x {ch}; texels={T}; chunks of {args.chunk} texels; a 2,000-step field is not a converged scene: the figures show the tool"]
if not n_f:
    lines.append("  no surface at any level tried: nothing is measured")
    finish(lines)
    sys.exit(0)

w, h, cpr = atlas_layout(n_f, T)
n = w * h
table = _tables(images, rpcs, dev, None, None)
view, to_sat = _view_tables(table, rpcs, min_alt, max_alt, offset, scale, zone, south, dev)
caster = MeshRaycaster(mesh)
bias = caster.default_bias()
face = torch.empty(n, dtype=torch.int32, device=dev)
xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
lla = torch.empty(n, 3, dtype=torch.float64, device=dev)
normal = torch.empty(n, 3, dtype=torch.float32, device=dev)
blocked = torch.empty(K, n, dtype=torch.uint8, device=dev)
colour = torch.empty(n, ch, dtype=torch.float32, device=dev)
wsum = torch.empty(n, dtype=torch.float32, device=dev)
count = torch.empty(n, dtype=torch.int32, device=dev)
best = torch.empty(n, dtype=torch.int32, device=dev)
sc, off = _f3(scale), _f3(offset)
chunks = [(first, min(args.chunk, n - first)) for first in range(0, n, args.chunk)]
structs = [_rpc_struct(r) for r in rpcs]
ones = (C.c_float * ch)(*([1.0] * ch))
zeros = (C.c_float * ch)(*([0.0] * ch))


def samples_leg():
    for first, m in chunks:
        _lib.check(L.eonerf_texture_samples(_ptr(vertices), n_v, _ptr(faces), n_f, T, first, m, sc, off, zone, 1 if south else 0, _ptr(face[first:]), None,
                                            _ptr(xyz[first:]), _ptr(lla[first:]), _ptr(normal[first:]), _stream()))


def occlusion_leg():
    for first, m in chunks:
        for k in range(K):
            blocked[k, first:first + m] = caster.occluded(xyz[first:first + m], (-view[k]).expand(m, 3).contiguous(), skip_face=face[first:first + m], t_min=bias)


def chunk_table(first, m):
    return blocked[:, first:first + m].contiguous() if len(chunks) > 1 else blocked


def bake_leg(with_normal, mode):
    def leg():
        for first, m in chunks:
            _bake(lla[first:first + m], normal[first:first + m] if with_normal else None, table, to_sat, chunk_table(first, m), 0.1, with_normal, mode,
                  colour[first:first + m], wsum[first:first + m], count[first:first + m], best[first:first + m])
    return leg


def baseline_leg(mode):
    def leg():
        for first, m in chunks:
            layers = torch.empty(K, m, ch, dtype=torch.float32, device=dev)
            weights = torch.empty(K, m, dtype=torch.float32, device=dev)
            for k in range(K):
                _lib.check(L.eonerf_ortho_gather(_ptr(lla[first:]), m, C.byref(structs[k]), _ptr(images[k]), args.side, args.side, ch, ones, zeros,
                                                 _ptr(visibility[k, first:]), 0.5, _ptr(layers[k]), _ptr(weights[k]), None, _stream()))
            _lib.check(L.eonerf_ortho_fuse(_ptr(layers), _ptr(weights), K, m, ch, mode, _ptr(colour[first:]), _ptr(wsum[first:]), _ptr(count[first:]), _stream()))
    return leg


with torch.no_grad():
    samples_leg()
    occlusion_leg()
visibility = (1.0 - blocked.float()).contiguous()        # the baseline's input, made outside its timing
owned = face >= 0
n_owned = int(owned.sum())
lines.append(f"  atlas {w} x {h} = {n} texels, {n_owned} owned by a face ({100 * n_owned / n:.1f} %); {int(blocked.sum())} of {K * n} (image, texel) pairs blocked at bias {bias:.3g}; "
             f"the K x n x C layers the baseline would hold unchunked: {K * n * ch * 4 / 2 ** 20:.0f} MiB + {K * n * 4 / 2 ** 20:.0f} MiB of weights")

# the fused bake without a normal against gather + fuse: the same bits, and the peak memory of each above what both share
same = {}
for name, mode in (("mean", 0), ("median", 1)):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        bake_leg(False, mode)()
    torch.cuda.synchronize()
    fused_peak = torch.cuda.max_memory_allocated() - before
    a = (colour.clone(), wsum.clone(), count.clone())
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        baseline_leg(mode)()
    torch.cuda.synchronize()
    base_peak = torch.cuda.max_memory_allocated() - torch.cuda.memory_allocated()
    same[name] = bool(a[0].view(torch.int32).equal(colour.view(torch.int32)) and a[1].view(torch.int32).equal(wsum.view(torch.int32)) and a[2].equal(count))
    lines.append(f"  {name}: fused bake (normal = NULL) and gather + fuse give the same colour, weight and count bits: {same[name]}; peak device memory above the shared tables: "
                 f"fused {fused_peak / 2 ** 20:.1f} MiB, gather + fuse {base_peak / 2 ** 20:.1f} MiB")
del a

torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
res = bake_texture(mesh, images, rpcs, offset, scale, zone, south, min_alt, max_alt, texels=T, raycaster=caster, chunk=args.chunk)
torch.cuda.synchronize()
textured = int(((res["count"].reshape(-1) > 0) & owned).sum()) / max(n_owned, 1)
lines.append(f"  bake_texture (median, occlusion, angle weight, min_cos 0.1): mesh/texels={n_owned} | mesh/textured={textured:.4f}; peak device memory of the call, the tables "
             f"of this script included: {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
del res

legs = {"samples": samples_leg, "occlusion casts (K per chunk)": occlusion_leg,
        "bake, product form (normals, angle weight, median)": bake_leg(True, 1),
        "bake, normal = NULL, median": bake_leg(False, 1), "baseline: K gathers + fuse, median": baseline_leg(1),
        "bake, normal = NULL, mean": bake_leg(False, 0), "baseline: K gathers + fuse, mean": baseline_leg(0)}
lines.append(f"time: alternating, {args.rounds} rounds after a warm-up of all; ms over the whole atlas, device events around work ending in one synchronise")
times = {name: [] for name in legs}
for leg in legs.values():
    timed(leg)
for _ in range(args.rounds):
    for name, leg in legs.items():
        times[name].append(timed(leg)[0])
for name in legs:
    lines.append(row(name, times[name], f"   {1e6 * stats(times[name])[0] / n:.2f} ns per texel"))
for name in ("median", "mean"):
    f_m, f_s = stats(times[f"bake, normal = NULL, {name}"])
    b_m, b_s = stats(times[f"baseline: K gathers + fuse, {name}"])
    verdict = "no longer than the baseline beyond the baseline's own spread" if f_m <= b_m + b_s else "LONGER than the baseline beyond its spread"
    lines.append(f"  {name}: fused {f_m:.3f} ms against {b_m:.3f} ms (max - min {b_s:.3f}) of gather + fuse: {b_m / f_m:.2f} x; the fused bake is {verdict}")
finish(lines)
