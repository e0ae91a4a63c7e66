#!/usr/bin/env python3
"""Generate tests/golden/g11_nadir.npz and g12_dsmr.npz by running the REFERENCE's own Python code (/root/reference, read-only)
on the CPU in the build container, in the manner of make_golden.py.  Never runs on the GPU box: only the .npz outputs travel.

Names of packages that are absent here are supplied by placeholder modules (no arithmetic): numba.jit as the identity
decorator (the reference's dsmr.py then runs as plain Python), and empty rasterio / torchvision / rpcm / nerfacc.

The rasters are handed to dsmr as float64 arrays that hold float32-representable values: under numba the accumulators of
mean_std / downsample2x_ type as float64 over a float32 raster, while in plain Python a float32 array would make them float32.

g11: create_rays_from_nadir / generate_rays_from_virtual_pinhole (eval_eonerf.py:78-95,130-249).
g12: dsmr.downsample2x / compute_ncc / recursive_ncc / mean_std / apply_shift_ on two GT / prediction pairs, and the error raster
     and MAE of sat_utils.py:181-185,201-207,255 (file I/O left out: those lines are re-typed in numpy below, on the arrays
     the reference's functions returned).

Usage:  python tests/golden/make_golden_dsm.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)          # must precede site-packages: a HuggingFace `datasets` package is installed


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Missing:
    def __init__(self, *a, **k):
        raise RuntimeError("placeholder for an un-vendored third-party symbol was called")


_placeholder("numba", jit=lambda f=None, **k: f if f is not None else (lambda g: g))
_placeholder("rasterio")
_placeholder("torchvision", transforms=_placeholder("torchvision.transforms"))
_placeholder("rpcm", RPCModel=_Missing)
_placeholder("nerfacc", OccGridEstimator=_Missing, rendering=_Missing, render_transmittance_from_density=_Missing,
             accumulate_along_rays=_Missing)
try:
    import PIL  # noqa: F401
except ImportError:
    _placeholder("PIL", Image=_placeholder("PIL.Image"))

import dsmr  # noqa: E402
import eval_eonerf as ref_eval  # noqa: E402

MAX_BYTES = 200 * 1000
MIN_LEAD = 1e-4


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    size = os.path.getsize(path)
    print(f"wrote {name}.npz, {size} bytes, {len(out)} arrays")
    assert size < MAX_BYTES, size


# ------------------------------------------------------------------ G11 nadir camera
def g11():
    scale = np.array([128.5, 131.25, 40.0], dtype=np.float32)
    suns = [(35.0, 160.0), (62.5, 220.0)]
    out = {"scene_scale": scale, "suns": np.array(suns), "sizes": np.array([[7, 5], [16, 24]]), "radius": 2.0, "near": 0.0, "far": 2.5,
           "el_az": np.array([[0.0, 0.0], [10.0, 135.0]])}
    dataset = types.SimpleNamespace(scene_scale=torch.from_numpy(scale.copy()), img_downscale=1)
    for h, w in ((7, 5), (16, 24)):
        for k, (sel, saz) in enumerate(suns):
            rays = ref_eval.create_rays_from_nadir(dataset, h, w, sel, saz)
            assert rays.dtype == torch.float32 and tuple(rays.shape) == (h * w, 11)
            out[f"nadir.{h}x{w}.sun{k}"] = rays.numpy()
        # an oblique virtual camera through the same function (8 columns: no sun direction)
        rays = ref_eval.generate_rays_from_virtual_pinhole(w, h, max(h, w), 2, 10.0, 135.0, 0, 2.5, scene_scale=scale.copy())
        assert rays.dtype == torch.float32 and tuple(rays.shape) == (h * w, 8)
        out[f"oblique.{h}x{w}"] = rays.numpy()
    save("g11_nadir", out)


# ------------------------------------------------------------------ G12 registration + MAE
def terrain(rng, H, W, n_boxes):
    yy, xx = np.mgrid[0:H + 16, 0:W + 16].astype(np.float64)
    base = 20 + 6 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    for _ in range(n_boxes):
        y0, x0 = rng.integers(0, H), rng.integers(0, W)
        base[y0:y0 + rng.integers(6, 18), x0:x0 + rng.integers(6, 18)] += rng.uniform(4, 25)
    return base


def make_pair(seed, gt_hw, pred_hw, shift, n_boxes):
    """GT = smooth terrain + boxes; prediction = GT displaced by `shift` px, + 1.7 m, sigma 0.3 m noise, 3 % NaN holes.  Values are
    rounded to 1/64 m (GT) and 1/256 m (prediction): float32-representable, and the fixture compresses."""
    rng = np.random.default_rng(seed)
    (H, W), (PH, PW) = gt_hw, pred_hw
    base = terrain(rng, max(H, PH), max(W, PW), n_boxes)
    dx, dy = shift
    gt = (np.round(base[8:8 + H, 8:8 + W] * 64) / 64).astype(np.float32)
    pred = base[8 + dy:8 + dy + PH, 8 + dx:8 + dx + PW] + 1.7 + rng.normal(0, 0.3, (PH, PW))
    pred = (np.round(pred * 256) / 256).astype(np.float32)
    pred[rng.random((PH, PW)) < 0.03] = np.nan
    return gt, pred


def scores_of(u, v, cx, cy):
    s = np.array([dsmr.ncc(u, v, x, y) for y in range(cy - 5, cy + 6) for x in range(cx - 5, cx + 6)], dtype=np.float64)
    top = np.sort(s[np.isfinite(s)])[::-1]
    assert top[0] - top[1] >= MIN_LEAD, (top[0], top[1])          # no near-tie may flip an argmax on another machine
    return s, float(top[0] - top[1])


def register(tag, gt, pred, out):
    """dsmr.compute_shift's body (:183-190) on arrays, level by level."""
    u, v = gt.astype(np.float64)[None], pred.astype(np.float64)[None]
    levels = [(u, v)]
    while min(levels[-1][0].shape[-1], levels[-1][0].shape[-2]) > 100:
        levels.append((dsmr.downsample2x(levels[-1][0]), dsmr.downsample2x(levels[-1][1])))
    dx, dy = dsmr.recursive_ncc(u, v)
    cx, cy = 0, 0
    for k in range(len(levels) - 1, -1, -1):
        lu, lv = levels[k]
        if k:
            out[f"{tag}.level{k}.ref"], out[f"{tag}.level{k}.sec"] = lu[0], lv[0]
        s, lead = scores_of(lu, lv, cx, cy)
        got = dsmr.compute_ncc(lu, lv, 5, cx, cy)
        out[f"{tag}.level{k}.centre"], out[f"{tag}.level{k}.shift"], out[f"{tag}.level{k}.scores"] = np.array([cx, cy]), np.array(got), s
        print(f"  {tag} level {k}: centre {(cx, cy)} -> {got}, lead {lead:.3e}")
        cx, cy = 2 * got[0], 2 * got[1]
    assert (dx, dy) == tuple(out[f"{tag}.level0.shift"])
    out[f"{tag}.n_levels"] = len(levels)
    stats = np.array(dsmr.mean_std(u, v, dx, dy), dtype=np.float64)              # muu, muv, sigu, sigv, xcorr
    out[f"{tag}.mean_std"] = stats
    muu, muv, sigu, sigv, _ = stats
    a_s = sigu / sigv
    out[f"{tag}.transform"] = np.array([dx, dy, 1.0, muu - muv * 1.0])           # scaling=False, as sat_utils.py:197 calls it
    out[f"{tag}.transform_scaling"] = np.array([dx, dy, a_s, muu - muv * a_s])
    print(f"  {tag}: (dx, dy) = {(dx, dy)}, b = {muu - muv:.6f}, a(scaling) = {a_s:.6f}")
    return dx, dy, 1.0, muu - muv * 1.0


def error_raster(tag, gt, pred, transform, out):
    dx, dy, a, b = transform
    shifted = np.zeros_like(pred)                                                # float32, as the GeoTIFF the reference writes
    dsmr.apply_shift_(pred.astype(np.float64)[None], shifted[None], int(dx), int(dy), a, b, 0, 0)
    # sat_utils.py:201-207
    h, w = min(shifted.shape[0], gt.shape[0]), min(shifted.shape[1], gt.shape[1])
    max_gt_alt, min_gt_alt = gt.max(), gt.min()
    clipped = np.clip(shifted, min_gt_alt - 10, max_gt_alt + 10)
    err = clipped[:h, :w] - gt[:h, :w]
    assert err.dtype == np.float32
    mae = np.nanmean(abs(err.ravel()))                                           # :255
    out[f"{tag}.shifted"], out[f"{tag}.err"] = shifted, err
    out[f"{tag}.mae"], out[f"{tag}.n_valid"] = np.float64(mae), int(np.isfinite(err).sum())
    print(f"  {tag}: mae {float(mae):.7f} over {int(np.isfinite(err).sum())} cells")


def g12():
    out = {}
    # pair A: 118 x 105 -> two levels (59 x 53 below), odd sizes at both
    gt, pred = make_pair(7, (118, 105), (118, 105), (3, -2), 14)
    out["a.gt"], out["a.pred"] = gt, pred
    tr = register("a", gt, pred, out)
    error_raster("a", gt, pred, tr, out)
    # pair B: sec larger than ref, one level; also with a water mask (sat_utils.py:181-185: masked BEFORE the registration)
    gt, pred = make_pair(11, (60, 70), (64, 76), (-2, 4), 8)
    out["b.gt"], out["b.pred"] = gt, pred
    tr = register("b", gt, pred, out)
    error_raster("b", gt, pred, tr, out)
    water = np.zeros((62, 72), dtype=np.uint8)                                   # a third shape: the mask covers a top-left part only
    water[20:34, 30:55] = 1
    water[50:62, 0:9] = 1
    masked = pred.copy()
    water_ = np.zeros_like(masked)
    h_, w_ = min(water.shape[0], masked.shape[0]), min(water.shape[1], masked.shape[1])
    water_[:h_, :w_] = water.astype(bool)[:h_, :w_]
    masked[water_.astype(bool)] = np.nan
    out["bw.water"], out["bw.masked"] = water, masked
    tr = register("bw", gt, masked, out)
    error_raster("bw", gt, masked, tr, out)
    out = {k: v for k, v in out.items() if k not in ("bw.masked", "bw.shifted", "b.shifted")}      # derivable; keeps the file small
    save("g12_dsmr", out)


if __name__ == "__main__":
    only = sys.argv[1:]
    for name, fn in (("g11", g11), ("g12", g12)):
        if not only or name in only:
            fn()
