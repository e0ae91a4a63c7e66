"""A/B of the quantile depth (include/eonerf_quantile.h; sat_rendering.render_depth_quantiles, evaluate_dsm(depth_quantile=)) on one GPU,
by the protocol of scripts/occ_ab.py / march_ab.py.  The scene: tests/bf16_common.twin_train -- the synthetic terrain, 2,000 steps in
bf16 -- rendered on the fp16x3 export context: one 512 x 512 nadir view (262,144 rays, chunk 5120) at 128 samples per ray.
Two measurements.
  time   the render leg: render_depth_quantiles with K = 1 (the median) and K = 5 quantiles against render_image(only_depth=True), the
         parent's code unchanged; the two alternate, three rounds after a warm-up of both, device events around work that ends in one
         synchronise; the baseline's own max - min is printed beside the ratio.
  MAE    evaluate_dsm against the terrain's own surface (tests/bf16_common.terrain_height on a 1 m grid): the expected depth against
         q = 0.3 / 0.5 / 0.7, each dense, with the default occupancy grid, and with early_stop_eps 0.25 at block 32; three jitter keys,
         mean and max - min over them.
    python3 scripts/quantile_ab.py [--out profiles/depth_quantile_ab.txt] [--side 512] [--rounds 3] [--steps 2000]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import STEP, Z_SCALE, terrain_height, twin_train
from eonerf_code_amd import dsm
from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
from eonerf_code_amd.occupancy import OccupancyGrid
from eonerf_code_amd.sat_rendering import render_depth_quantiles, render_image

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--resolution", type=int, default=128)
args = ap.parse_args()

CHUNK, NS, KEYS = 5120, 128, (7, 8, 9)
SC, OFF = [250.0, 250.0, Z_SCALE], [10250.0, 50250.0, 20.0]      # the cube spans 500 m; positive UTM coordinates
SIZE, RES, SUN = 400, 1.0, (35.0, 160.0)
ROI = (OFF[0] - 0.5 * SIZE * RES, OFF[1] - 0.5 * SIZE * RES, SIZE, RES)
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
# the terrain's own surface on the ROI's grid (cell centres; row 0 is the northern edge)
c = (torch.arange(SIZE, dtype=torch.float64) + 0.5) * RES
x = (ROI[0] + c - OFF[0]) / SC[0]
y = (ROI[1] + SIZE * RES - c - OFF[1]) / SC[1]
gt = (OFF[2] + SC[2] * terrain_height(x[None, :], y[:, None])).float().to(dev)
rays = dsm.nadir_rays(args.side, args.side, SC, *SUN, device=dev)
sat = define_satrays_from_tensors(rays, torch.zeros(rays.shape[0], 1, dtype=torch.int64, device=dev))
n_rays = rays.shape[0]
QS5 = (0.02, 0.16, 0.5, 0.84, 0.98)


def baseline():
    field.set_noise_seed(KEYS[0])
    return render_image(field, None, sat, None, None, chunk=CHUNK, render_step_size=STEP, only_depth=True, eval=True)


def quantile_leg(qs):
    def run():
        field.set_noise_seed(KEYS[0])
        return render_depth_quantiles(field, None, sat, qs, chunk=CHUNK, render_step_size=STEP)
    return run


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


lines = [f"quantile depth A/B: {args.side} x {args.side} nadir view ({n_rays} rays, chunk {CHUNK}), {NS} samples per ray; twin_train bf16 field, {args.steps} steps, "
         f"{field.eval_precision} export context",
         f"time: baseline = render_image(only_depth=True) (the parent's code path); alternating, {args.rounds} rounds after a warm-up of both; ms per render, "
         "device events around work ending in one synchronise"]
for tag, qs in (("K = 1 (0.5)", (0.5,)), ("K = 5 (0.02, 0.16, 0.5, 0.84, 0.98)", QS5)):
    leg = quantile_leg(qs)
    (_, (b_res, b_n)), (_, (q_res, q_n)) = timed(baseline), timed(leg)      # warm-up of both
    assert torch.equal(b_res["depth"], q_res["depth"]) and b_n == q_n       # the expected depth is the baseline's, bit for bit
    b, g = [], []
    for _ in range(args.rounds):
        b.append(timed(baseline)[0])
        g.append(timed(leg)[0])
    (bm, bs), (gm, gs) = stats(b), stats(g)
    verdict = "within the baseline's spread" if abs(gm - bm) <= bs else ("slower" if gm > bm else "faster") + " by more than the baseline's spread"
    lines.append(f"{tag}: baseline {' '.join(f'{v:8.2f}' for v in b)} (median {bm:.2f}, max - min {bs:.2f}) | quantiles {' '.join(f'{v:8.2f}' for v in g)} "
                 f"(median {gm:.2f}, max - min {gs:.2f}) | ratio {gm / bm:.3f} | {verdict}")
    print(lines[-1], flush=True)
band = (q_res["depth_q"][:, 3] - q_res["depth_q"][:, 1]) * Z_SCALE
lines.append(f"16 % .. 84 % band of the view: median {band.median().item():.3f} m, p99 {band.quantile(0.99).item():.3f} m; od_front median "
             f"{q_res['od_front'].median().item():.3f}; |median - expected| altitude: mean {((q_res['depth_q'][:, 2] - q_res['depth'][:, 0]).abs() * Z_SCALE).mean().item():.3f} m")

grid = OccupancyGrid(args.resolution, device=dev)
field.train()      # (build runs on the training context; keep the module's state as the trainer has it)
grid.build(field, STEP)
field.eval()
lines.append(f"DSM MAE against the terrain's own surface ({SIZE} x {SIZE} cells of {RES:g} m), registered as evaluate_dsm does; jitter keys {KEYS}: mean (max - min) in m")
MODES = (("dense", dict()), ("default grid", dict(occupancy_grid=grid)), ("early_stop_eps 0.25, block 32", dict(early_stop_eps=0.25, march_block=32)))
table = {}
for mode, kw in MODES:
    row = []
    for q in (None, 0.3, 0.5, 0.7):
        v = []
        for key in KEYS:
            field.set_noise_seed(key)
            v.append(float(dsm.evaluate_dsm(field, gt, ROI, OFF, SC, SUN, chunk=CHUNK, render_step_size=STEP, h=args.side, w=args.side, depth_quantile=q, **kw)[0]))
        table[(mode, q)] = sum(v) / len(v)
        row.append(f"{'expected' if q is None else f'q = {q:g}'}: {sum(v) / len(v):.4f} ({max(v) - min(v):.4f})")
    lines.append(f"  {mode}: " + " | ".join(row))
    print(lines[-1], flush=True)
for q in (None, 0.3, 0.5, 0.7):
    d = [abs(table[(mode, q)] - table[("dense", q)]) for mode, _ in MODES[1:]]
    lines.append(f"  {'expected' if q is None else f'q = {q:g}'}: MAE moved against dense by {d[0]:.4f} m (grid), {d[1]:.4f} m (early termination)")
best = min((0.3, 0.5, 0.7), key=lambda q: table[("dense", q)])
lines.append(f"dense: the best quantile is q = {best:g} with {table[('dense', best)]:.4f} m against {table[('dense', None)]:.4f} m of the expected depth: "
             + ("the quantile lowers the MAE" if table[("dense", best)] < table[("dense", None)] else "the quantile does NOT lower the MAE"))
assert field.eval_precision == "fp16x3", "the export context fell back to fp32: the figures above mix precisions"
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
