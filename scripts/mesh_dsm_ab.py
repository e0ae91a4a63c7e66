"""The mesh on the scale of the DSM MAE (include/eonerf_mesh_dsm.h; eonerf_code_amd/mesh.py rasterize_mesh / evaluate_mesh_dsm) on one GPU,
by the protocol of scripts/mesh_ab.py.  The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- with the
terrain's own surface as the lidar DSM, as scripts/quantile_ab.py builds it, on a --side x --side grid (512) under the normalised cube.
  * the DSM MAE of the expected depth, of the median depth (dsm.evaluate_dsm) and of the mesh DSM (mesh.evaluate_mesh_dsm) of a
    --res^3 extraction (256) at the default level: three read-outs of one field;
  * the mesh DSM's MAE over the level: level_from_opacity(alpha, 2 / 128) for alpha = 0.1 .. 0.9;
  * the mesh DSM's MAE over min_component_points (0, 8, 64, 512) and with fill_cavities, at the default level;
  * the rasteriser's time beside the density volume and the depth-only nadir render: the legs alternate, --rounds rounds after a warm-up of
    all, device events around work that ends in one synchronise; a rasteriser leg is --repeat calls back to back in one window and the
    table shows the window over --repeat; max - min beside the median;
  * the same for the coarse-mesh regime, a 9^3 extraction on a 2048^2 grid, where a few hundred triangles cover all the cells and every
    one is walked by a whole wave; time per covered cell of both regimes side by side.
The sweep is the tool a converged checkpoint is read with; a 2,000-step field decides no default.
    python3 scripts/mesh_dsm_ab.py [--out profiles/mesh_dsm_ab.txt] [--rounds 3] [--steps 2000] [--res 256] [--side 512] [--repeat 100]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import STEP, Z_SCALE, terrain_height, twin_train
from eonerf_code_amd import _lib, dsm
from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
from eonerf_code_amd.mesh import density_volume, evaluate_mesh_dsm, filter_components, lattice_of, level_from_opacity, mesh_from_volume
from eonerf_code_amd._lib import _ptr, _stream
from eonerf_code_amd.sat_rendering import render_image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--repeat", type=int, default=100)
args = ap.parse_args()

CHUNK, SUN = 5120, (35.0, 160.0)
SC, OFF = [250.0, 250.0, Z_SCALE], [10250.0, 50250.0, 20.0]      # the cube spans 500 m; positive UTM coordinates
SIZE = args.side
RES = 460.0 / SIZE                                                # the grid spans 460 m: every cell lies under the cube
ROI = (OFF[0] - 0.5 * SIZE * RES, OFF[1] - 0.5 * SIZE * RES, SIZE, RES)
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
L = _lib.lib()
c = (torch.arange(SIZE, dtype=torch.float64) + 0.5) * RES
x = (ROI[0] + c - OFF[0]) / SC[0]
y = (ROI[1] + SIZE * RES - c - OFF[1]) / SC[1]
gt = (OFF[2] + SC[2] * terrain_height(x[None, :], y[:, None])).float().to(dev)
DEFAULT = level_from_opacity(0.5, 2.0 / 128)


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
    return f"  {tag:<28}{' '.join(f'{t:9.3f}' for t in v)}   median {m:9.3f} ms, max - min {s:.3f}{extra}"


def mesh_mae(volume, level, origin, spacing, **filters):
    report = None
    if filters:
        volume, report = filter_components(volume, level, **filters)
    v, t = mesh_from_volume(volume, level, origin, spacing)
    if t.shape[0] == 0:
        return None, 0, 0, None, report
    out = evaluate_mesh_dsm((v, t), gt, ROI, OFF, SC, return_all=True)
    mae, cells = out["mae"].tolist()
    return mae, t.shape[0], int(cells), out["transform"].tolist(), report


def raster_leg(v, t, grid):
    """--repeat calls of eonerf_mesh_dsm_rasterize on buffers allocated beforehand."""
    xoff, yoff, xs, ys, res = grid
    keys = torch.empty(xs * ys, dtype=torch.int64, device=dev)
    out = torch.empty(ys, xs, dtype=torch.float32, device=dev)
    face = torch.empty(ys, xs, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    sc, of = dsm._d3(SC), dsm._d3(OFF)

    def leg():
        for _ in range(args.repeat):
            _lib.check(L.eonerf_mesh_dsm_rasterize(_ptr(v), v.shape[0], _ptr(t), t.shape[0], sc, of, xoff, yoff, xs, ys, res, _ptr(keys), _ptr(out),
                                                   _ptr(face), _ptr(counts), _stream()))
        return counts
    return leg


lines = [f"mesh DSM: twin_train bf16 field, {args.steps} steps, {field.eval_precision} export context; lidar DSM = the terrain's own surface on {SIZE} x {SIZE} cells of "
         f"{RES:g} m; registered as evaluate_dsm does; a 2,000-step field is not a converged scene: the figures show the tool, they decide no default"]
origin, spacing = lattice_of(args.res)
volume = density_volume(field, args.res)
rays = dsm.nadir_rays(SIZE, SIZE, SC, *SUN, device=dev)
sat = define_satrays_from_tensors(rays, torch.zeros(rays.shape[0], 1, dtype=torch.int64, device=dev))
exp = float(dsm.evaluate_dsm(field, gt, ROI, OFF, SC, SUN, chunk=CHUNK, render_step_size=STEP, h=SIZE, w=SIZE)[0])
med = float(dsm.evaluate_dsm(field, gt, ROI, OFF, SC, SUN, chunk=CHUNK, render_step_size=STEP, h=SIZE, w=SIZE, depth_quantile=0.5)[0])
mae, n_t, cells, tr, _ = mesh_mae(volume, DEFAULT, origin, spacing)
lines.append(f"three read-outs of one field (DSM MAE in m): expected depth {exp:.4f} | median depth {med:.4f} | mesh DSM, {args.res}^3 at the default level "
             f"{DEFAULT:.4f}: " + (f"{mae:.4f} ({n_t} triangles, {cells} of {SIZE * SIZE} cells valid, shift dx {tr[0]:g} dy {tr[1]:g} b {tr[3]:.4f})" if mae is not None else "no surface at this level"))
lines.append(f"level sweep, {args.res}^3, level_from_opacity(alpha, 2 / 128):")
for k in range(1, 10):
    alpha = k / 10
    level = level_from_opacity(alpha, 2.0 / 128)
    mae, n_t, cells, tr, _ = mesh_mae(volume, level, origin, spacing)
    lines.append(f"  alpha {alpha:.1f}  level {level:9.4f}  " + (f"MAE {mae:8.4f} m   {n_t:9d} triangles   {cells:7d} cells valid   b {tr[3]:8.4f}" if mae is not None else "no surface"))
lines.append(f"clean-up at the default level, {args.res}^3:")
for tag, kw in [(f"min_component_points={m}", {"min_points": m}) for m in (0, 8, 64, 512)] + [("fill_cavities", {"fill_cavities": True})]:
    kw = {k: v for k, v in kw.items() if v}
    mae, n_t, cells, tr, report = mesh_mae(volume, DEFAULT, origin, spacing, **kw)
    lines.append(f"  {tag:<26}" + (f"MAE {mae:8.4f} m   {n_t:9d} triangles   {cells:7d} cells valid" if mae is not None else "no surface") +
                 (f"   ({', '.join(f'{k} {v}' for k, v in report.items())})" if report else ""))
print("\n".join(lines), flush=True)
shown = len(lines)

# ---- time -----------------------------------------------------------------------------------------------------------------------
lines.append(f"time: alternating, {args.rounds} rounds after a warm-up of all; the rasteriser as {args.repeat} calls per window (time per call: two memsets, the "
             "triangle launch, the resolve launch); ms, device events around work ending in one synchronise")
v_fine, t_fine = mesh_from_volume(volume, DEFAULT, origin, spacing)
level_fine = DEFAULT
if t_fine.shape[0] == 0:                                  # a young field may not reach the default level: the densest level that has a surface
    for k in range(9, 0, -1):
        level_fine = level_from_opacity(k / 10, 2.0 / 128)
        v_fine, t_fine = mesh_from_volume(volume, level_fine, origin, spacing)
        if t_fine.shape[0]:
            break
coarse_volume = density_volume(field, 9)
o9, s9 = lattice_of(9)
level_coarse, v_coarse, t_coarse = None, None, None
for k in range(5, 0, -1):
    level_coarse = level_from_opacity(k / 10, 2.0 / 128)
    v_coarse, t_coarse = mesh_from_volume(coarse_volume, level_coarse, o9, s9)
    if t_coarse.shape[0]:
        break
grid_fine = dsm.grid_from_roi(ROI)
grid_coarse = dsm.grid_from_roi((OFF[0] - 230.0, OFF[1] - 230.0, 2048, 460.0 / 2048))
legs = {"density volume": lambda: density_volume(field, args.res),
        "depth-only nadir render": lambda: render_image(field, None, sat, None, None, chunk=CHUNK, render_step_size=STEP, only_depth=True, eval=True)}
if t_fine.shape[0]:
    legs["rasteriser, fine"] = raster_leg(v_fine, t_fine, grid_fine)
if t_coarse is not None and t_coarse.shape[0]:
    legs["rasteriser, coarse"] = raster_leg(v_coarse, t_coarse, grid_coarse)
times, last = {k: [] for k in legs}, {}
for leg in legs.values():
    timed(leg)
for _ in range(args.rounds):
    for name, leg in legs.items():
        ms, last[name] = timed(leg)
        times[name].append(ms / (args.repeat if name.startswith("rasteriser") else 1))
lines.append(row(f"density volume {args.res}^3", times["density volume"]))
lines.append(row(f"nadir render {SIZE}^2", times["depth-only nadir render"]))
per_cell = {}
for name, t, grid, level in (("rasteriser, fine", t_fine, grid_fine, level_fine), ("rasteriser, coarse", t_coarse, grid_coarse, level_coarse)):
    if name not in legs:
        lines.append(f"  {name}: no surface to rasterise at any level tried: unmeasured")
        continue
    cnt = last[name].tolist()
    m = stats(times[name])[0]
    per_cell[name] = 1e6 * m / max(cnt[3], 1)
    lines.append(row(name, times[name], f"   {t.shape[0]} triangles (level {level:.4f}) on {grid[2]} x {grid[3]}: {cnt[0]} rasterised, {cnt[1]} dropped, {cnt[2]} degenerate, "
                                        f"{cnt[3]} cells covered; {per_cell[name]:.3f} ns per covered cell, {1e6 * m / max(t.shape[0], 1):.3f} ns per triangle"))
if "rasteriser, fine" in legs:
    m = stats(times["rasteriser, fine"])[0]
    lines.append(f"  the rasteriser is {100 * m / stats(times['density volume'])[0]:.2f} % of the density volume it reads and {100 * m / stats(times['depth-only nadir render'])[0]:.2f} % of the "
                 "nadir render it stands beside")
if len(per_cell) == 2:
    ratio = per_cell["rasteriser, coarse"] / per_cell["rasteriser, fine"]
    lines.append(f"  per covered cell the coarse regime takes {ratio:.2f} x the fine one" +
                 (": more than an order of magnitude -- a few hundred triangles occupy a handful of waves, each walking its triangles one after the other, "
                  "while the rest of the device idles" if ratio > 10 else ""))
print("\n".join(lines[shown:]), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
