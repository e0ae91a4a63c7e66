"""Dual contouring (csrc/eonerf_dual.h; mesh.dual_contour) beside marching tetrahedra (include/eonerf_mesh.h) on one GPU, by the
protocol of scripts/mesh_ab.py and scripts/smooth_ab.py.  The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in
bf16 -- sampled on the export context on a --res^3 lattice over the normalised cube.
Timed on the same volume at the default level: eonerf_dual_count, eonerf_dual_hermite, normals.density_gradient at the Hermite points
and eonerf_dual_emit, beside eonerf_mesh_count, eonerf_mesh_emit and density_gradient at marching tetrahedra's vertices (what
extract_mesh's normals cost there; a dual mesh asks for that again at its own, fewer, vertices: the row "normals at the dual vertices").
Buffers are allocated beforehand; the legs alternate, --rounds rounds after a warm-up of all, device events around work that ends in one
synchronise; a library call is tens of microseconds, so such a leg is --repeat calls back to back and the table shows the window over
--repeat.  Then the vertex and triangle counts, dual_contour's report, and mesh/mae (mesh.evaluate_mesh_dsm against the terrain's own
surface) for marching tetrahedra and for dual contouring at lambda 0.03, 0.1 and 0.3.
There is no gate: a 2,000-step field is not a converged scene, and no default changes on the strength of these figures.
    python3 scripts/dual_ab.py [--out profiles/dual_ab.txt] [--rounds 3] [--steps 2000] [--res 256] [--side 512] [--repeat 20]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import Z_SCALE, terrain_height, twin_train
from eonerf_code_amd import _lib
from eonerf_code_amd._lib import _ptr, _stream
from eonerf_code_amd.mesh import MeshDict, density_volume, dual_contour, evaluate_mesh_dsm, lattice_of, level_from_opacity, mesh_from_volume
from eonerf_code_amd.normals import density_gradient

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeat", type=int, default=20)
args = ap.parse_args()

SC, OFF = [250.0, 250.0, Z_SCALE], [10250.0, 50250.0, 20.0]      # the cube spans 500 m; positive UTM coordinates
SIZE = args.side
RES = 460.0 / SIZE
ROI = (OFF[0] - 0.5 * SIZE * RES, OFF[1] - 0.5 * SIZE * RES, SIZE, RES)
LAMBDAS = (0.03, 0.1, 0.3)
CHUNK = 1 << 20
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
L = _lib.lib()
c = (torch.arange(SIZE, dtype=torch.float64) + 0.5) * RES
gt = (OFF[2] + SC[2] * terrain_height(((ROI[0] + c - OFF[0]) / SC[0])[None, :], ((ROI[1] + SIZE * RES - c - OFF[1]) / SC[1])[:, None])).float().to(dev)


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


def mae_of(vertices, faces):
    if faces.shape[0] == 0:
        return "no surface"
    mesh = MeshDict({"vertices": vertices, "faces": faces})
    mae, cells = evaluate_mesh_dsm(mesh, gt, ROI, OFF, SC).tolist()
    return f"{mae:.4f} m ({int(cells)} cells valid)"


def gradient_at(points):
    parts = [density_gradient(field, points[i:i + CHUNK])[1] for i in range(0, points.shape[0], CHUNK)]
    return torch.cat(parts, dim=0) if parts else points.new_empty(0, 3)


n_side = args.res
origin, spacing = lattice_of(n_side)
volume = density_volume(field, n_side)
level = level_from_opacity(0.5, 2.0 / 128)
tv, tt = mesh_from_volume(volume, level, origin, spacing)
if tt.shape[0] == 0:                                      # a young field may not reach the default level: the densest level that has a surface
    for a in range(9, 0, -1):
        level = level_from_opacity(a / 10, 2.0 / 128)
        tv, tt = mesh_from_volume(volume, level, origin, spacing)
        if tt.shape[0]:
            break
dv, dt, report, _, points, _ = dual_contour(volume, level, gradient_at, origin, spacing, return_keys=True)
n_h, n_v, n_t = points.shape[0], dv.shape[0], dt.shape[0]
lines = [f"dual contouring beside marching tetrahedra: twin_train bf16 field, {args.steps} steps, {field.eval_precision} export context; {n_side}^3 lattice at level "
         f"{level:.4f}; alternating, {args.rounds} rounds after a warm-up of all, library calls as {args.repeat} calls per window (time per call); ms, device events "
         "around work ending in one synchronise; a 2,000-step field is not a converged scene: the figures show the tool, they decide no default",
         f"  marching tetrahedra: {tv.shape[0]:9d} vertices, {tt.shape[0]:9d} triangles",
         f"  dual contouring:     {n_v:9d} vertices, {n_t:9d} triangles, {n_h} Hermite points ({n_t / max(tt.shape[0], 1):.3f} x the triangles); report at lambda 0.1: "
         + ", ".join(f"{k}={report[k]}" for k in ("clamped", "fallback", "dropped_planes", "nonfinite_edges"))]

nb_t, nb_d = L.eonerf_mesh_workspace_bytes(n_side, n_side, n_side), L.eonerf_dual_workspace_bytes(n_side, n_side, n_side)
ws_t, ws_d = torch.empty(nb_t, dtype=torch.uint8, device=dev), torch.empty(nb_d, dtype=torch.uint8, device=dev)
counts_t, counts_d = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
vert_t, tri_t = torch.empty(max(tv.shape[0], 1), 3, dtype=torch.float32, device=dev), torch.empty(max(tt.shape[0], 1), 3, dtype=torch.int32, device=dev)
pts = torch.empty(max(n_h, 1), 3, dtype=torch.float32, device=dev)
vert_d, tri_d = torch.empty(max(n_v, 1), 3, dtype=torch.float32, device=dev), torch.empty(max(n_t, 1), 3, dtype=torch.int32, device=dev)
status, rep = torch.empty(1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
grad = gradient_at(points)
g_in = grad if n_h else torch.zeros(1, 3, dtype=torch.float32, device=dev)
dims = (n_side, n_side, n_side)


def many(call):
    def leg():
        for _ in range(args.repeat):
            _lib.check(call())
    return leg


legs = [
    ("tetra count", many(lambda: L.eonerf_mesh_count(_ptr(volume), *dims, level, _ptr(counts_t), _ptr(ws_t), nb_t, _stream())), args.repeat),
    ("tetra emit", many(lambda: L.eonerf_mesh_emit(_ptr(volume), *dims, level, origin, spacing, _ptr(ws_t), nb_t, _ptr(vert_t), tv.shape[0], _ptr(tri_t), tt.shape[0],
                                                   None, _ptr(status), _stream())), args.repeat),
    ("tetra normals (gradient at its vertices)", lambda: gradient_at(tv), 1),
    ("dual count", many(lambda: L.eonerf_dual_count(_ptr(volume), *dims, level, _ptr(counts_d), _ptr(ws_d), nb_d, _stream())), args.repeat),
    ("dual hermite", many(lambda: L.eonerf_dual_hermite(_ptr(volume), *dims, level, origin, spacing, _ptr(ws_d), nb_d, _ptr(pts), n_h, None, _ptr(status), _stream())), args.repeat),
    ("dual gradient (at the Hermite points)", lambda: gradient_at(points), 1),
    ("dual emit", many(lambda: L.eonerf_dual_emit(_ptr(volume), *dims, level, origin, spacing, _ptr(g_in), n_h, 0.1, _ptr(ws_d), nb_d, _ptr(vert_d), n_v, None, _ptr(tri_d), n_t,
                                                  _ptr(rep), _ptr(status), _stream())), args.repeat),
    ("normals at the dual vertices", lambda: gradient_at(dv), 1),
]
for _, leg, _ in legs:                                    # warm-up of all
    timed(leg)
assert counts_t.tolist()[:2] == [tv.shape[0], tt.shape[0]] and counts_d.tolist()[:3] == [n_h, n_v, n_t] and int(status.item()) == 0
assert torch.equal(vert_d[:n_v], dv) and torch.equal(tri_d[:n_t], dt)
times = {tag: [] for tag, _, _ in legs}
for _ in range(args.rounds):
    for tag, leg, per in legs:
        times[tag].append(timed(leg)[0] / per)
for tag, _, _ in legs:
    lines.append(row(tag, times[tag]))
med = {tag: stats(v)[0] for tag, v in times.items()}
tetra = med["tetra count"] + med["tetra emit"] + med["tetra normals (gradient at its vertices)"]
dual = med["dual count"] + med["dual hermite"] + med["dual gradient (at the Hermite points)"] + med["dual emit"]
lines.append(f"  marching tetrahedra, count + emit + normals: {tetra:.3f} ms;  dual contouring, count + hermite + gradient + emit: {dual:.3f} ms, with normals at its "
             f"own vertices {dual + med['normals at the dual vertices']:.3f} ms")
lines.append(f"  mesh/mae  marching tetrahedra: {mae_of(tv, tt)}")
for lam in LAMBDAS:
    v, t, r = dual_contour(volume, level, grad, origin, spacing, regularisation=lam)
    lines.append(f"  mesh/mae  dual contouring, lambda {lam:<5g}: {mae_of(v, t)}; clamped={r['clamped']}, fallback={r['fallback']}, dropped_planes={r['dropped_planes']}")
print("\n".join(lines), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
