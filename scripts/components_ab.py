"""Timing of the mesh clean-up (include/eonerf_components.h; eonerf_code_amd/mesh.py) on one GPU, by the protocol of scripts/mesh_ab.py.
The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- sampled on the fp16x3 export context on lattices of
128^3 and 256^3 points over the normalised cube, at the default level of extract_mesh.
Per lattice: the time of the density volume (mesh.density_volume, the yardstick the labelling consumes), of eonerf_cc_label (inside
components; all its launches) and of eonerf_cc_filter, buffers allocated beforehand, and of the host path the feature replaces: the
volume read back, scipy.ndimage.label with the 15-voxel structure of the seven directions on the host's threads, the labels uploaded.
The legs alternate, three rounds after a warm-up of all, device events around work that ends in one synchronise (the host leg: wall
clock around the same); max - min is printed beside the median.  A label or filter leg is --repeat calls back to back in one window and
the table shows the window over --repeat: the time per call, launch gaps included.
Per stage: the device time of every kernel of one more window of --repeat label calls and --repeat filter calls, from torch.profiler's
kernel records (mean per launch), with the bytes the stage has to move and the rate that makes, beside the measured HBM copy rate of the
MI355X (6.29 TB/s; 8 TB/s is the specification):
    bytes(local)   = 4 n (the volume, once) + 8 n (labels and info, written)
    bytes(merge)   = 4 n x (share of the points on a forward face of their tile)
    bytes(flatten) = 8 n (labels and info, read) -- what it writes back depends on the scene and is not counted
    bytes(counts)  = 4 n (labels)
    bytes(filter)  = 8 n (volume and labels, read) + 4 n (volume, written)
Walks of the parent array and the gathers of info at roots are not counted: they depend on the scene.
Then the scene itself: components, their sizes by decade, and vertices / triangles of the mesh under each filter.
    python3 scripts/components_ab.py [--out profiles/components_ab.txt] [--rounds 3] [--steps 2000] [--sizes 128 256] [--repeat 10]"""
import argparse
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

from bf16_common import twin_train
from eonerf_code_amd import _lib
from eonerf_code_amd.mesh import (COUNT_MASK, UNIT_CUBE, density_volume, filter_components, lattice_of, level_from_opacity, mesh_from_volume)
from eonerf_code_amd._lib import _ptr, _stream

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--repeat", type=int, default=10)
args = ap.parse_args()

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
L = _lib.lib()
LEVEL = level_from_opacity(0.5, 2.0 / 128)
hdr = open(os.path.join(REPO, "include", "eonerf_components.h")).read()
TX, TY, TZ = (int(re.search(r"#define\s+EONERF_CC_TILE_%s\s+(\d+)" % a, hdr).group(1)) for a in "XYZ")
try:
    from scipy import ndimage
except ImportError:
    ndimage = None
STRUCTURE = np.zeros((3, 3, 3), dtype=bool)
STRUCTURE[1, 1, 1] = True
for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
    STRUCTURE[1 + dz, 1 + dy, 1 + dx] = STRUCTURE[1 - dz, 1 - dy, 1 - dx] = True


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def stats(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def row(tag, v, extra=""):
    m, s = stats(v)
    return f"  {tag:<16}{' '.join(f'{x:9.3f}' for x in v)}   median {m:9.3f} ms, max - min {s:.3f}{extra}"


def rate(nbytes, ms):
    return f"{nbytes / 1e6:9.2f} MB -> {nbytes / ms / 1e9:7.3f} TB/s ({100 * nbytes / ms / 1e9 / (HBM_MEASURED / 1e12):.1f} % of the measured HBM rate)"


lines = [f"mesh clean-up: twin_train bf16 field, {args.steps} steps; alternating, {args.rounds} rounds after a warm-up of all, label and filter as {args.repeat} calls per window (time per call); ms, device events around work ending in one synchronise",
         f"HBM beside the rates: {HBM_MEASURED / 1e12:.2f} TB/s measured copy rate, {HBM_SPEC / 1e12:.1f} TB/s specification; tiles of {TX} x {TY} x {TZ} points; "
         f"host path: scipy {'missing' if ndimage is None else 'present'}, {os.environ.get('OMP_NUM_THREADS', '?')} host threads allowed"]
shown = 0
for n_side in args.sizes:
    n = n_side ** 3
    origin, spacing = lattice_of(n_side, UNIT_CUBE)
    volume = density_volume(field, n_side)
    lines.append(f"{n_side}^3 lattice points ({n} points), export context {field.eval_precision}, level {LEVEL:.4f}")
    nb = L.eonerf_cc_workspace_bytes(n_side, n_side, n_side)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    labels = torch.empty(n_side, n_side, n_side, dtype=torch.int32, device=dev)
    info = torch.empty_like(labels)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    dropped = torch.empty(2, dtype=torch.int64, device=dev)
    f_out = torch.empty_like(volume)

    def volume_leg():
        return density_volume(field, n_side)

    def label_leg():
        for _ in range(args.repeat):
            _lib.check(L.eonerf_cc_label(_ptr(volume), n_side, n_side, n_side, LEVEL, 0, _ptr(labels), _ptr(info), _ptr(counts), _ptr(ws), nb, _stream()))

    def filter_leg():
        for _ in range(args.repeat):
            _lib.check(L.eonerf_cc_filter(_ptr(volume), _ptr(labels), _ptr(info), n_side, n_side, n_side, 0, 64, 0, _ptr(f_out), _ptr(dropped), _stream()))

    def host_leg():
        host = volume.cpu().numpy()
        lab, n_comp = ndimage.label(host >= np.float32(LEVEL), structure=STRUCTURE)
        return n_comp, torch.from_numpy(lab).to(dev)

    legs = [volume_leg, label_leg, filter_leg]
    for leg in legs:                                    # warm-up of all
        timed(leg)
    n_comp, n_points, largest, root = counts.tolist()
    host_comp = None
    if ndimage is not None:
        host_comp = wall(host_leg)[1][0]
        assert host_comp == n_comp, (host_comp, n_comp)
    tv, tl, tf, th = [], [], [], []
    for _ in range(args.rounds):
        tv.append(timed(volume_leg)[0])
        tl.append(timed(label_leg)[0] / args.repeat)
        tf.append(timed(filter_leg)[0] / args.repeat)
        if ndimage is not None:
            th.append(wall(host_leg)[0])
    mv, ml, mf = stats(tv)[0], stats(tl)[0], stats(tf)[0]
    face = 1.0 - (1 - 1 / TX) * (1 - 1 / TY) * (1 - 1 / TZ)
    stage_bytes = {"k_cc_local": 12 * n, "k_cc_merge": int(4 * n * face), "k_cc_flatten": 8 * n, "k_cc_counts": 4 * n, "k_cc_finish": 8, "k_cc_filter": 12 * n}
    lines.append(row("density volume", tv, f"   {n / mv / 1e3:8.2f} M points/s"))
    lines.append(row("label", tl, f"   {rate(sum(stage_bytes[k] for k in stage_bytes if k != 'k_cc_filter'), ml)}"))
    lines.append(row("filter", tf, f"   {rate(stage_bytes['k_cc_filter'], mf)}"))
    lines.append(f"  label = {100 * ml / mv:.2f} % of the density volume it consumes; label + filter = {ml + mf:.3f} ms = {100 * (ml + mf) / mv:.2f} %")
    if th:
        mh = stats(th)[0]
        lines.append(row("host path", th, f"   read-back + scipy.ndimage.label (14 neighbours) + upload, wall clock; {mh / ml:.0f} x the label call; {host_comp} components on both paths"))
    else:
        lines.append("  host path: scipy is not installed here, so the path the feature replaces was not measured")
    # per stage: one more window under the profiler
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            label_leg()
            filter_leg()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.events():
            m = re.search(r"k_cc_[a-z]+", ev.name or "")
            if m:
                per.setdefault(m.group(0), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        lines.append(f"  per stage (device time of the kernel alone, mean of {args.repeat} launches under torch.profiler):")
        for name in ("k_cc_local", "k_cc_merge", "k_cc_flatten", "k_cc_counts", "k_cc_finish", "k_cc_filter"):
            if name in per:
                ms = sum(per[name]) / len(per[name]) / 1e3
                lines.append(f"    {name[5:]:<10}{ms:9.4f} ms ({len(per[name])} launches)   {rate(stage_bytes[name], ms) if name != 'k_cc_finish' else ''}")
        if not per:
            lines.append("    the profiler returned no kernel records: the stages were not measured separately")
    except Exception as exc:                            # the profiler is optional equipment: say so, keep the rest
        lines.append(f"  per stage: torch.profiler failed ({type(exc).__name__}: {exc}); the stages were not measured separately")
    # the scene
    sizes = (info.reshape(-1) & COUNT_MASK)
    sizes = sizes[sizes > 0]
    touching = int((info.reshape(-1) < 0).sum())
    lines.append(f"  scene: {n_comp} inside components, {n_points} inside points; largest {largest} points at root {root}, "
                 f"{'touches' if int(info.reshape(-1)[root]) < 0 else 'does not touch'} the boundary; {touching} component(s) touch the boundary")
    decades = torch.floor(torch.log10(sizes.double())).long()
    lines.append("  sizes by decade: " + ", ".join(f"10^{d}..: {int((decades == d).sum())}" for d in range(int(decades.max()) + 1)))
    second = int(torch.topk(sizes, min(2, sizes.numel())).values[-1]) if sizes.numel() > 1 else 0
    lines.append(f"  second largest component: {second} points")
    v, t = mesh_from_volume(volume, LEVEL, origin, spacing)
    lines.append(f"  mesh unfiltered:            {v.shape[0]:9d} vertices, {t.shape[0]:9d} triangles")
    for tag, kw in [(f"min_points={m}", {"min_points": m}) for m in (8, 64, 512)] + [("keep_largest=1", {"keep_largest": 1}), ("fill_cavities", {"fill_cavities": True})]:
        out, report = filter_components(volume, LEVEL, **kw)
        v, t = mesh_from_volume(out, LEVEL, origin, spacing)
        lines.append(f"  mesh {tag:<22} {v.shape[0]:9d} vertices, {t.shape[0]:9d} triangles   ({', '.join(f'{k} {x}' for k, x in report.items())})")
        del out
    print("\n".join(lines[shown:]), flush=True)
    shown = len(lines)
    del volume, ws, labels, info, f_out
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
