"""Ray casting against a mesh (eonerf_code_amd/csrc/eonerf_raycast.h; eonerf_code_amd/mesh.py MeshRaycaster, render_mesh) on one GPU,
by the protocol of scripts/smooth_ab.py.  The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- meshed on
a --res^3 lattice (256) at the default level (or the densest level that has a surface).  The view: --side^2 rays (512), a regular grid of
origins over the scene at the height the training rays start from, one oblique direction that converges slightly, one sun.
  * per grid of 32, 64, 128 and 256 cells an axis: the list entries and the workspace, the time of eonerf_raycast_count, of
    eonerf_raycast_build, of eonerf_raycast_closest over the view and of eonerf_raycast_occluded over the shadow rays of its hits (from the
    hit points towards the sun -- against the table's sun column --, skipping their own face, at the default bias) -- --repeat calls back to back in one window, buffers
    allocated beforehand, no read-back;
  * the depth-only export render_image of the same rays, in the same run;
  * mesh/view_depth and mesh/shadow_agree of that view (mesh.mesh_view_metrics), and that every grid gives the same bits.
The legs alternate, --rounds rounds after a warm-up of all; device events around work that ends in one synchronise; max - min beside the
median.  The fastest grid (closest + occluded, the build once per mesh left aside) is named at the end: mesh.RAYCAST_DEFAULT_DIM follows it.
A 2,000-step field decides nothing else.
    python3 scripts/raycast_ab.py [--out profiles/raycast_ab.txt] [--rounds 3] [--steps 2000] [--res 256] [--side 512] [--repeat 20]"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import twin_train
from eonerf_code_amd import _lib
from eonerf_code_amd._lib import _ptr, _stream
from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
from eonerf_code_amd.mesh import MeshDict, MeshRaycaster, density_volume, lattice_of, level_from_opacity, mesh_from_volume, mesh_view_metrics
from eonerf_code_amd.sat_rendering import render_image
from eonerf_code_amd.synthetic import synthetic_batch
from eonerf_code_amd.validation import _step_size_of

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeat", type=int, default=20)
ap.add_argument("--dims", type=int, nargs="+", default=[32, 64, 128, 256])
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
    return f"  {tag:<40}{' '.join(f'{t:9.3f}' for t in v)}   median {m:9.3f} ms, max - min {s:.3f}{extra}"


origin, spacing = lattice_of(args.res)
volume = density_volume(field, args.res)
level = level_from_opacity(0.5, 2.0 / 128)
v, t = mesh_from_volume(volume, level, origin, spacing)
if t.shape[0] == 0:                                       # a young field may not reach the default level: the densest level that has a surface
    for a in range(9, 0, -1):
        level = level_from_opacity(a / 10, 2.0 / 128)
        v, t = mesh_from_volume(volume, level, origin, spacing)
        if t.shape[0]:
            break
del volume
mesh = MeshDict({"vertices": v, "faces": t})
mesh.lattice = {"origin": tuple(origin), "spacing": tuple(spacing), "shape": (args.res,) * 3}
n_v, n_t = v.shape[0], t.shape[0]

# the view: a regular grid of origins, one oblique direction converging slightly towards the scene's centre, the sun of a training image
S = args.side
c = (torch.arange(S, dtype=torch.float32) + 0.5) / S * 1.8 - 0.9
yy, xx = torch.meshgrid(c, c, indexing="ij")
o = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.full((S * S,), 0.98)], 1)
d = torch.stack([0.12 - 0.03 * o[:, 0], -0.08 - 0.03 * o[:, 1], -torch.ones(S * S)], 1)
d = d / d.norm(dim=1, keepdim=True)
sun = synthetic_batch(4, 5)[0][0, 8:11]
rays = torch.cat([o, d, torch.zeros(S * S, 1), 2 * torch.ones(S * S, 1), sun.expand(S * S, 3)], 1).to(dev).contiguous()
sat = define_satrays_from_tensors(rays, torch.zeros(S * S, 1, dtype=torch.int64, device=dev))
to_sun = (-rays[:, 8:11]).contiguous()                    # the column holds the direction the light travels
step_size = _step_size_of(field)
n = S * S

lines = [f"mesh ray casting: twin_train bf16 field, {args.steps} steps, {field.eval_precision} export context; {args.res}^3 lattice at level {level:.4f}: {n_v} vertices, "
         f"{n_t} triangles; the view: {S} x {S} rays from z = 0.98, oblique and slightly converging, sun {[round(float(x), 4) for x in sun]}; a 2,000-step field is "
         "not a converged scene: the figures show the tool, they decide the default grid and nothing else"]
if not n_t:
    lines.append("  no surface at any level tried: nothing is measured")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)

casters, legs, results = {}, {}, {}
t_out = torch.empty(n, dtype=torch.float64, device=dev)
face = torch.empty(n, dtype=torch.int32, device=dev)
bary = torch.empty(n, 3, dtype=torch.float32, device=dev)
blocked = torch.empty(n, dtype=torch.uint8, device=dev)
counts = torch.zeros(3, dtype=torch.int64, device=dev)
legs["depth-only render_image"] = (lambda: render_image(field, None, sat, None, None, render_step_size=step_size, only_depth=True, eval=True), 1)
for dim in args.dims:
    caster = casters[dim] = MeshRaycaster(mesh, dims=dim)
    near = caster.closest(rays[:, 0:3], rays[:, 3:6])
    point = (rays[:, 0:3].double() + near["t"].unsqueeze(-1) * rays[:, 3:6].double()).float().contiguous()
    bias = caster.default_bias()
    shade = caster.occluded(point, to_sun, skip_face=near["face"], t_min=bias)
    results[dim] = (near, shade)
    head = (_ptr(caster._v), n_v, _ptr(caster._f), n_t, caster._lo, caster._hi, caster._dims)
    cells = dim ** 3
    cell_counts = torch.empty(cells, dtype=torch.int32, device=dev)
    built = torch.zeros(2, dtype=torch.int64, device=dev)
    skip = near["face"].contiguous()

    def count_leg(head=head, cell_counts=cell_counts, built=built):
        for _ in range(args.repeat):
            _lib.check(L.eonerf_raycast_count(*head, _ptr(cell_counts), _ptr(built), _stream()))

    def build_leg(head=head, cell_counts=cell_counts, caster=caster):
        for _ in range(args.repeat):
            _lib.check(L.eonerf_raycast_build(*head, _ptr(cell_counts), caster.entries, _ptr(caster._ws), caster._ws.numel(), _stream()))

    def closest_leg(head=head, caster=caster):
        for _ in range(args.repeat):
            _lib.check(L.eonerf_raycast_closest(*head, caster.entries, _ptr(caster._ws), caster._ws.numel(), _ptr(rays), 11, C.c_void_p(rays.data_ptr() + 12), 11, n, 0.0,
                                                float("inf"), _ptr(t_out), _ptr(face), _ptr(bary), _ptr(counts), _stream()))

    def occluded_leg(head=head, caster=caster, point=point, skip=skip, bias=bias):
        for _ in range(args.repeat):
            _lib.check(L.eonerf_raycast_occluded(*head, caster.entries, _ptr(caster._ws), caster._ws.numel(), _ptr(point), 3, _ptr(to_sun), 3, n, bias,
                                                 float("inf"), _ptr(skip), _ptr(blocked), _ptr(counts), _stream()))

    count_leg()                                            # the cell counts the build leg scans
    legs[f"{dim}^3 count"] = (count_leg, args.repeat)
    legs[f"{dim}^3 build"] = (build_leg, args.repeat)
    legs[f"{dim}^3 closest"] = (closest_leg, args.repeat)
    legs[f"{dim}^3 occluded"] = (occluded_leg, args.repeat)

base = results[args.dims[0]]
same = all(r[0]["t"].view(torch.int64).equal(base[0]["t"].view(torch.int64)) and r[0]["face"].equal(base[0]["face"]) and r[0]["bary"].view(torch.int32).equal(base[0]["bary"].view(torch.int32))
           and r[1].equal(base[1]) for r in results.values())
hits = int(base[0]["hit"].sum())
lines.append(f"  {hits} of {n} rays hit; {int(base[1].sum())} of their shadow rays are blocked (bias {casters[args.dims[0]].default_bias():.3g}); every grid gives the same t, "
             f"face, bary and shadow bits: {same}")
for dim, caster in casters.items():
    lines.append(f"  {dim}^3: {caster.entries} list entries = {caster.entries / max(n_t - caster.dropped, 1):.2f} per triangle, {caster.dropped} dropped, workspace "
                 f"{caster._ws.numel() / 2 ** 20:.1f} MiB + {4 * dim ** 3 / 2 ** 20:.1f} MiB of cell counts")
metrics = mesh_view_metrics(field, mesh, [{"rays": rays}], raycaster=casters[args.dims[-1]]).tolist()
lines.append(f"  mesh/view_depth={metrics[0]:.5f} (scene units; the cube spans 2) | mesh/view_hits={int(metrics[1])} | mesh/view_rays={int(metrics[3])} | "
             f"mesh/shadow_agree={metrics[2]:.4f}")
print("\n".join(lines), flush=True)
shown = len(lines)

lines.append(f"time: alternating, {args.rounds} rounds after a warm-up of all; raycast legs as {args.repeat} calls per window on buffers allocated beforehand (time per call); "
             "ms, device events around work ending in one synchronise")
times = {name: [] for name in legs}
for leg, _ in legs.values():
    timed(leg)
for _ in range(args.rounds):
    for name, (leg, repeat) in legs.items():
        times[name].append(timed(leg)[0] / repeat)
render_ms = stats(times["depth-only render_image"])[0]
for name in legs:
    m = stats(times[name])[0]
    extra = "" if name.startswith("depth") else f"   {100 * m / render_ms:.2f} % of the depth-only render" + (f", {1e6 * m / n:.2f} ns per ray" if "closest" in name or "occluded" in name else "")
    lines.append(row(name, times[name], extra))
cast = {dim: stats(times[f"{dim}^3 closest"])[0] + stats(times[f"{dim}^3 occluded"])[0] for dim in args.dims}
best = min(cast, key=cast.get)
lines.append("  closest + occluded per view: " + ", ".join(f"{dim}^3 {ms:.3f} ms" for dim, ms in cast.items()) + f"; count + build once per mesh: " +
             ", ".join(f"{dim}^3 {stats(times[f'{dim}^3 count'])[0] + stats(times[f'{dim}^3 build'])[0]:.3f} ms" for dim in args.dims))
lines.append(f"  the fastest measured grid is {best}^3: closest + occluded take {cast[best]:.3f} ms against {render_ms:.3f} ms of the field's depth-only render of the same rays "
             f"({render_ms / cast[best]:.1f} x); mesh.RAYCAST_DEFAULT_DIM = {best}")
print("\n".join(lines[shown:]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
