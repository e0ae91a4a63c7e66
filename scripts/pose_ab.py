"""A/B of the camera offset refinement (include/eonerf_pose.h; FusedTrainer(origin_offsets=True)) on one GPU: the benchmark's full step
(4096 rays x 128 samples, bf16, shadow pass + uncertainty loss, in-kernel jitter) with and without the origin gradient, two trainers over
fields of the same weights in one process, in alternating blocks behind a warm-up of both.  Device events around each block; a block ends
in one synchronise.  Printed: the per-block step times of both, the ratio of their medians, the baseline's own max - min, and -- events
around the call itself, in a separate pass so that they do not sit in the timed blocks -- the time of the origin-gradient call (its
three launches: the MFMA tail over the camera tiles, the per-ray and the per-image sums) and of the rest of the offsets' bookkeeping
(apply_origin_offsets, the torch Adam of the table).  Nothing is asserted.
    python3 scripts/pose_ab.py [--out profiles/pose_ab.txt] [--blocks 6] [--steps 40]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

from eonerf_code_amd import pose
from eonerf_code_amd.radiance_fields.eonerf import EONerfMLP
from eonerf_code_amd.synthetic import synthetic_batch
from eonerf_code_amd.trainer import FusedTrainer, RayTable

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()

RAYS, N_IMG, EPOCH = 4096, 19, 3
dev = torch.device("cuda", 0)
torch.manual_seed(42)
base = EONerfMLP(N_IMG, radiometric_normalization=True, precision="bf16").to(dev)
sd = {k: v.clone() for k, v in base.state_dict().items()}
trainers = {}
for name, on in (("off", False), ("on", True)):
    f = EONerfMLP(N_IMG, radiometric_normalization=True, precision="bf16").to(dev)
    f.load_state_dict(sd)
    trainers[name] = FusedTrainer(f, lr=5e-4, max_rays=RAYS, keep_message=False, origin_offsets=on)
    trainers[name].set_noise_seed(42)
table = RayTable(*synthetic_batch(RAYS * 16, N_IMG, seed=1234), dev, seed=42)
spe = table.steps_per_epoch(RAYS)


def block(tr, first, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        r, im, px = table.batch(0, (first + i) % spe, RAYS)
        tr.step(r, im, px, EPOCH)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


lines = []
for tr in trainers.values():
    block(tr, 0, 20)
times = {"off": [], "on": []}
for b in range(args.blocks):
    for name in (("off", "on") if b % 2 == 0 else ("on", "off")):
        times[name].append(block(trainers[name], b * args.steps, args.steps))
for tr in trainers.values():
    tr.check_device_status()
med = {k: statistics.median(v) for k, v in times.items()}
lines.append(f"full step, {RAYS} rays x 128 samples, bf16, {args.blocks} alternating blocks of {args.steps} steps (ms per step)")
for k in ("off", "on"):
    lines.append(f"  offsets {k:3s}: " + " ".join(f"{t:.4f}" for t in times[k]) + f" | median {med[k]:.4f} | max - min {max(times[k]) - min(times[k]):.4f}")
lines.append(f"  step ratio on / off (medians): {med['on'] / med['off']:.4f}; baseline spread / median: {(max(times['off']) - min(times['off'])) / med['off']:.4f}")

# the pieces, outside the timed blocks
tr = trainers["on"]
real = pose.origin_grad
spans = {"origin_grad": [], "apply": [], "adam": []}


def timed(key, fn):
    def run(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn(*a, **kw)
        e1.record()
        spans[key].append((e0, e1))
        return res
    return run


import eonerf_code_amd.trainer as trainer_mod
trainer_mod.origin_grad = timed("origin_grad", real)
trainer_mod.apply_origin_offsets = timed("apply", pose.apply_origin_offsets)
tr._step_offsets = timed("adam", tr._step_offsets)
block(tr, 0, 30)
for key, ev in spans.items():
    us = [a.elapsed_time(b) * 1e3 for a, b in ev[5:]]
    lines.append(f"  {key:12s}: median {statistics.median(us):.1f} us, min {min(us):.1f} us over {len(us)} steps (device events around the call)")
lines.append(f"  pose/max_offset after the run: {float(pose.max_offset(tr.origin_offsets)):.6g}")
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
