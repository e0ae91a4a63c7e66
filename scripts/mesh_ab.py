"""Timing of the mesh export (include/eonerf_mesh.h; eonerf_code_amd/mesh.py) on one GPU, by the protocol of scripts/normals_ab.py.
The scene: tests/bf16_common.twin_train -- the synthetic terrain, trained in bf16 -- sampled on the fp16x3 export context on lattices of
128^3 and 256^3 points over the normalised cube.
Per lattice: the time of the density volume (mesh.density_volume), of eonerf_mesh_count and of eonerf_mesh_emit separately, buffers
allocated beforehand; the three alternate, three rounds after a warm-up of all, device events around work that ends in one synchronise;
max - min is printed beside the median.  One mesh call is tens of microseconds, so a leg of count or emit is --repeat (20) calls back to
back in one window and the table shows the window over 20: the time per call, launch gaps included.  Then vertex and triangle counts at three levels, and the bytes the two mesh calls have to move
(computed from the shapes and counts below) per second, beside the measured HBM copy rate of the MI355X (6.29 TB/s; 8 TB/s is the
specification).
    bytes(count) = 4 n (the volume, once) + 5 n (two uint16 scans and the mask per point) + 3 x 8 n / 1024 (tile sums: written, scanned)
    bytes(emit)  = 4 n (the volume, once) + n (the masks) + 20 V (a vertex and its key) + 12 T (a triangle)
The lookups of emit around the surface (scans and masks of the seven neighbours, the volume's values again for each vertex) hit lines
another lane has just loaded; they are not counted.
    python3 scripts/mesh_ab.py [--out profiles/mesh_ab.txt] [--rounds 3] [--steps 2000] [--sizes 128 256] [--repeat 20]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

from bf16_common import twin_train
from eonerf_code_amd import _lib
from eonerf_code_amd.mesh import UNIT_CUBE, density_volume, lattice_of, level_from_opacity, mesh_from_volume
from eonerf_code_amd._lib import _ptr, _stream

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--repeat", type=int, default=20)
args = ap.parse_args()

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
dev = torch.device("cuda", 0)
field = twin_train("bf16", steps=args.steps)
field.eval()
L = _lib.lib()
LEVELS = [(a, level_from_opacity(a, 2.0 / 128)) for a in (0.1, 0.5, 0.9)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(v):
    return sorted(v)[len(v) // 2], max(v) - min(v)


def row(tag, v, extra=""):
    m, s = stats(v)
    return f"  {tag:<16}{' '.join(f'{x:9.3f}' for x in v)}   median {m:9.3f} ms, max - min {s:.3f}{extra}"


lines = [f"mesh export: twin_train bf16 field, {args.steps} steps; alternating, {args.rounds} rounds after a warm-up of all, count and emit as {args.repeat} calls per window (time per call); ms, device events around work ending in one synchronise",
         f"HBM beside the rates: {HBM_MEASURED / 1e12:.2f} TB/s measured copy rate, {HBM_SPEC / 1e12:.1f} TB/s specification"]
shown = 0
for n_side in args.sizes:
    n = n_side ** 3
    origin, spacing = lattice_of(n_side, UNIT_CUBE)
    volume = density_volume(field, n_side)              # warm-up of the volume leg; also the volume the mesh legs read
    lines.append(f"{n_side}^3 lattice points ({n} points), export context {field.eval_precision}; density min {float(volume.min()):.4g}, "
                 f"median {float(volume.median()):.4g}, max {float(volume.max()):.4g}")
    sizes = {}
    for alpha, level in LEVELS:
        v, t = mesh_from_volume(volume, level, origin, spacing)
        sizes[alpha] = (v.shape[0], t.shape[0])
        lines.append(f"  level {level:9.4f} (opacity {alpha} over a step of 2 / 128): {v.shape[0]:9d} vertices, {t.shape[0]:9d} triangles")
    alpha, level = LEVELS[1]
    n_v, n_t = sizes[alpha]
    nb = L.eonerf_mesh_workspace_bytes(n_side, n_side, n_side)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    vert = torch.empty(max(n_v, 1), 3, dtype=torch.float32, device=dev)
    tri = torch.empty(max(n_t, 1), 3, dtype=torch.int32, device=dev)
    key = torch.empty(max(n_v, 1), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)

    def volume_leg():
        return density_volume(field, n_side)

    def count_leg():
        for _ in range(args.repeat):
            _lib.check(L.eonerf_mesh_count(_ptr(volume), n_side, n_side, n_side, level, _ptr(counts), _ptr(ws), nb, _stream()))

    def emit_leg():
        for _ in range(args.repeat):
            _lib.check(L.eonerf_mesh_emit(_ptr(volume), n_side, n_side, n_side, level, origin, spacing, _ptr(ws), nb, _ptr(vert), n_v, _ptr(tri), n_t,
                                          _ptr(key), _ptr(status), _stream()))

    for leg in (volume_leg, count_leg, emit_leg):       # warm-up of all
        timed(leg)
    assert counts.tolist()[:2] == [n_v, n_t] and int(status.item()) == 0
    tv, tc, te = [], [], []
    for _ in range(args.rounds):
        tv.append(timed(volume_leg)[0])
        tc.append(timed(count_leg)[0] / args.repeat)
        te.append(timed(emit_leg)[0] / args.repeat)
    b_count = 4 * n + 5 * n + 3 * 8 * ((n + 1023) // 1024)
    b_emit = 4 * n + n + 20 * n_v + 12 * n_t
    mv, mc, me = stats(tv)[0], stats(tc)[0], stats(te)[0]
    lines.append(f"  at level {level:.4f}:")
    lines.append(row("density volume", tv, f"   {n / mv / 1e3:8.2f} M points/s"))
    lines.append(row("count", tc, f"   {b_count / 1e6:9.2f} MB -> {b_count / mc / 1e9:7.3f} TB/s ({100 * b_count / mc / 1e9 / (HBM_MEASURED / 1e12):.1f} % of the measured HBM rate)"))
    lines.append(row("emit", te, f"   {b_emit / 1e6:9.2f} MB -> {b_emit / me / 1e9:7.3f} TB/s ({100 * b_emit / me / 1e9 / (HBM_MEASURED / 1e12):.1f} % of the measured HBM rate)"))
    lines.append(f"  count + emit = {mc + me:.3f} ms = {100 * (mc + me) / mv:.2f} % of the density volume they consume")
    print("\n".join(lines[shown:]), flush=True)
    shown = len(lines)
    del volume, ws, vert, tri, key
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
