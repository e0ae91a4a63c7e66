"""A/B of relight.render_sun_sweep against the path it replaces -- K render_image calls with the sun columns of the ray table
overwritten -- on one GPU: a bf16 field (fp16x3 export context), 128 samples per ray, a 512 x 512 synthetic view (262,144 rays, chunk
5120), K in {1, 4, 8, 24}.  Both paths run in the same library; baseline and sweep alternate, three rounds after a warm-up of both; each
timing is taken with device events around work that ends in a synchronise.  The clock probe (eonerf_clock_probe) runs before and after.
    python3 scripts/sweep_ab.py [--out profiles/sun_sweep_ab.txt] [--side 512] [--rounds 3] [--ks 1,4,8,24]
    python3 scripts/sweep_ab.py --one 8          # one K = 8 sweep after a warm-up, nothing else (the run rocprofv3 --kernel-trace --stats wraps)"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

from eonerf_code_amd import _lib
from eonerf_code_amd.datasets.satellite import define_satrays_from_tensors
from eonerf_code_amd._lib import _ptr, _stream
from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
from eonerf_code_amd.relight import render_sun_sweep, sun_table
from eonerf_code_amd.sat_rendering import render_image
from eonerf_code_amd.synthetic import synthetic_batch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--ks", default="1,4,8,24")
ap.add_argument("--one", type=int, default=0)
args = ap.parse_args()

N_IMG, STEP, CHUNK = 19, 2.0 / 128, 5120
dev = torch.device("cuda", 0)
torch.manual_seed(42)
field = EONerfMLP(N_IMG, radiometric_normalization=True, precision="bf16").to(dev)
with torch.no_grad():      # a surface inside the cube, so that camera and shadow rays carry a realistic number of samples
    field.sigma_layer.output_layer.bias += 1.0
field.eval()
rays, img, _ = (t.to(dev).contiguous() for t in synthetic_batch(args.side * args.side, N_IMG, seed=1234))
img[:] = 0      # one view
sat = define_satrays_from_tensors(rays, img[:, None])
field.set_noise_seed(7)


def suns_of(k):
    # a day: the sun climbs and turns
    el = [15.0 + 60.0 * (i + 0.5) / k for i in range(k)]
    az = [90.0 + 180.0 * (i + 0.5) / k for i in range(k)]
    return sun_table(el, az, [1.0, 1.0, 1.0], device=dev)


def baseline(suns):
    """the parent's path: one render_image per sun on a table with columns 8..10 overwritten"""
    n = 0
    table = rays.clone()
    for k in range(suns.shape[0]):
        table[:, 8:11] = suns[k]
        res, c = render_image(field, None, define_satrays_from_tensors(table, img[:, None]), None, None, epoch_idx=3, chunk=CHUNK,
                              render_step_size=STEP, eval=True)
        n += c
    return n


def sweep(suns):
    res, c = render_sun_sweep(field, sat, suns, chunk=CHUNK, render_step_size=STEP, eval=True)
    return c


def timed(fn, suns):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with torch.no_grad():
        fn(suns)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def clock():
    out = torch.zeros(4, device=dev)
    _lib.check(_lib.lib().eonerf_clock_probe(field._context(), _ptr(out), _stream()))
    torch.cuda.synchronize()
    return out[2].item(), out[1].item() * 0.01


if args.one:
    s = suns_of(args.one)
    timed(sweep, s[:1])
    ms = timed(sweep, s)
    print(f"one K = {args.one} sweep: {ms:.2f} ms ({field.eval_precision} export context)")
    sys.exit(0)

lines = [f"sun sweep A/B: {args.side} x {args.side} view ({rays.shape[0]} rays, chunk {CHUNK}), 128 samples per ray, bf16 field, {field.eval_precision} export context",
         "baseline = K render_image calls with the sun columns overwritten; sweep = one render_sun_sweep; alternating, "
         f"{args.rounds} rounds after a warm-up of both; ms per series, device events around work ending in a synchronise"]
mhz, us = clock()
lines.append(f"clock probe before: {mhz:.0f} MHz ({us:.1f} us)")
for K in [int(k) for k in args.ks.split(",")]:
    s = suns_of(K)
    timed(baseline, s[:1]), timed(sweep, s[:1])      # warm-up of both (allocations, the export context's weights)
    if K > 1:
        timed(baseline, s), timed(sweep, s)
    b, w = [], []
    for _ in range(args.rounds):
        b.append(timed(baseline, s))
        w.append(timed(sweep, s))
    bm, wm = sorted(b)[len(b) // 2], sorted(w)[len(w) // 2]
    verdict = "faster by more than the baseline's spread" if bm - wm > max(b) - min(b) else "NOT faster by more than the baseline's spread"
    lines.append(f"K = {K:2d}: baseline {' '.join(f'{x:8.2f}' for x in b)} (median {bm:.2f}, max - min {max(b) - min(b):.2f}) | "
                 f"sweep {' '.join(f'{x:8.2f}' for x in w)} (median {wm:.2f}, max - min {max(w) - min(w):.2f}) | ratio {wm / bm:.3f} | {verdict}")
    print(lines[-1], flush=True)
mhz, us = clock()
lines.append(f"clock probe after: {mhz:.0f} MHz ({us:.1f} us)")
assert field.eval_precision == "fp16x3", "the export context fell back to fp32: the figures above mix precisions"
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
