"""numpy fp64 restatements of the DSM evaluation contract (include/eonerf_dsm.h), for shapes the goldens do not cover.

Written from the header's contract and checked against the reference's recorded outputs (tests/golden/g11_nadir.npz, g12_dsmr.npz)
by tests/test_dsm_restated_cpu.py.  Vectorised: sums are numpy's pairwise sums, so scores agree with a sequential fp64 sum to ~1e-12,
not to the bit; every integer result (shifts, NaN patterns, counts) is exact.
"""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- nadir camera
def dir_vec_from_el_az(elevation_deg, azimuth_deg):
    el, az = np.radians(90.0 - elevation_deg), np.radians(azimuth_deg)
    return -1.0 * np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)])


def nadir_rays(h, w, radius, elevation_deg, azimuth_deg, near, far, scene_scale, sun_elevation_deg, sun_azimuth_deg):
    """-> float32 [h*w, 11]: origins on the plane through (0,0,-1) - radius*d perpendicular to d, one direction d, near, far, sun."""
    scale = np.asarray(scene_scale, dtype=np.float64)
    d = dir_vec_from_el_az(elevation_deg, azimuth_deg) / scale
    d = d / np.linalg.norm(d)
    pt_a = np.array([0.0, 0.0, -1.0]) - radius * d
    x = (np.arange(w) - w * 0.5) / (w / radius) + pt_a[0]
    y = -(np.arange(h) - h * 0.5) / (h / radius) + pt_a[1]
    X, Y = np.meshgrid(x, y)
    Z = ((-d[0] * (X - pt_a[0]) - d[1] * (Y - pt_a[1])) / d[2]) + pt_a[2]
    sun = dir_vec_from_el_az(sun_elevation_deg, sun_azimuth_deg) / scale
    sun = sun / np.linalg.norm(sun)
    n = h * w
    view = d / np.linalg.norm(d)
    cols = [X.ravel(), Y.ravel(), Z.ravel()] + [np.full(n, c) for c in view] + [np.full(n, float(near)), np.full(n, float(far))]
    cols += [np.full(n, c) for c in sun]
    return np.stack(cols, axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- rasteriser
def grid_from_roi(roi):
    """(x, y, size, res) of a <aoi>_DSM.txt -> (xoff, yoff of the UPPER edge, xsize, ysize, res)."""
    xoff, yoff, size, res = float(roi[0]), float(roi[1]), int(roi[2]), float(roi[3])
    return xoff, yoff + size * res, size, size, res


def cloud_of(rays, depth, scale, offset):
    """Points (east, north, altitude) fp64 and the mask of the rays that are kept."""
    rays, depth = np.asarray(rays, dtype=np.float64), np.asarray(depth, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        xyz = (rays[:, 0:3] + rays[:, 3:6] * depth[:, None]) * np.asarray(scale, dtype=np.float64) + np.asarray(offset, dtype=np.float64)
        keep = np.isfinite(depth) & (depth >= 0) & np.isfinite(xyz[:, 0]) & np.isfinite(xyz[:, 1]) & (np.abs(xyz[:, 2]) < 2.0 ** 31)
    xyz = xyz.copy()
    neg = keep & (xyz[:, 1] < 0)
    xyz[neg, 1] += 10e6
    return xyz, keep


def grid_from_cloud(xyz, res):
    """The grid the reference derives from the cloud's extent when no ROI is given."""
    xmin, xmax, ymin, ymax = xyz[:, 0].min(), xyz[:, 0].max(), xyz[:, 1].min(), xyz[:, 1].max()
    xoff = np.floor(xmin / res) * res
    xsize = int(1 + np.floor((xmax - xoff) / res))
    yoff = np.ceil(ymax / res) * res
    ysize = int(1 - np.floor((ymin - yoff) / res))
    return float(xoff), float(yoff), xsize, ysize, float(res)


def rasterize(rays, depth, scale, offset, xoff, yoff, xsize, ysize, res):
    """-> (dsm float64 [ysize, xsize] = exact mean per cell or NaN, count int64): radius-1, weight-1 splat."""
    xyz, keep = cloud_of(rays, depth, scale, offset)
    xyz = xyz[keep]
    ci = np.floor((xyz[:, 0] - xoff) / res)
    cj = np.floor((yoff - xyz[:, 1]) / res)
    near = (ci >= -1) & (ci <= xsize) & (cj >= -1) & (cj <= ysize)
    ci, cj, alt = ci[near].astype(np.int64), cj[near].astype(np.int64), xyz[near, 2]
    total = np.zeros((ysize, xsize), dtype=np.float64)
    count = np.zeros((ysize, xsize), dtype=np.int64)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            j, i = cj + dj, ci + di
            ok = (j >= 0) & (j < ysize) & (i >= 0) & (i < xsize)
            np.add.at(total, (j[ok], i[ok]), alt[ok])
            np.add.at(count, (j[ok], i[ok]), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dsm = np.where(count > 0, total / count, np.nan)
    return dsm, count


# ---------------------------------------------------------------------------------------------------------------- registration
def downsample2x(u):
    """out[J, I] = mean of the finite values in the 2x2 window whose corner is (min(2J+1, h-1), min(2I+1, w-1)); fp64."""
    u = np.asarray(u, dtype=np.float64)
    h, w = u.shape
    pad = np.full((h + 1, w + 1), np.nan)
    pad[:h, :w] = u
    j = np.minimum(2 * np.arange((h + 1) // 2) + 1, h - 1)
    i = np.minimum(2 * np.arange((w + 1) // 2) + 1, w - 1)
    total = np.zeros((len(j), len(i)))
    count = np.zeros((len(j), len(i)), dtype=np.int64)
    for k in (0, 1):
        for l in (0, 1):
            t = pad[np.ix_(j + l, i + k)]
            ok = np.isfinite(t)
            total = total + np.where(ok, t, 0.0)
            count += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, total / count, np.nan)


def shifted(v, shape, dx, dy):
    """w[j, i] = v[j+dy, i+dx] over `shape`, NaN outside v."""
    v = np.asarray(v, dtype=np.float64)
    out = np.full(shape, np.nan)
    j0, j1 = max(0, -dy), min(shape[0], v.shape[0] - dy)
    i0, i1 = max(0, -dx), min(shape[1], v.shape[1] - dx)
    if j1 > j0 and i1 > i0:
        out[j0:j1, i0:i1] = v[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    return out


def mean_std(u, v, dx=0, dy=0):
    """-> muu, muv, sigu, sigv, xcorr over the pixels where u and the shifted v are both finite (NaN everywhere if there is none)."""
    u = np.asarray(u, dtype=np.float64)
    vs = shifted(v, u.shape, dx, dy)
    ok = np.isfinite(u) & np.isfinite(vs)
    n = int(ok.sum())
    if n == 0:
        return (math.nan,) * 5
    muu, muv = u[ok].sum() / n, vs[ok].sum() / n
    cu, cv = u[ok] - muu, vs[ok] - muv
    return muu, muv, math.sqrt((cu * cu).sum() / n), math.sqrt((cv * cv).sum() / n), (cu * cv).sum() / n


def ncc_scores(u, v, cx, cy, irange=5):
    """The (2*irange+1)^2 scores in scan order (y outer, x inner)."""
    out = []
    for y in range(cy - irange, cy + irange + 1):
        for x in range(cx - irange, cx + irange + 1):
            _, _, sigu, sigv, xcorr = mean_std(u, v, x, y)
            with np.errstate(invalid="ignore", divide="ignore"):
                out.append(np.float64(xcorr) / (np.float64(sigu) * np.float64(sigv)))
    return np.array(out, dtype=np.float64)


def pick(scores, cx, cy, irange=5):
    """First strict maximum in scan order; NaN never wins; the centre if nothing does."""
    dx, dy, maxv, n = cx, cy, -math.inf, 2 * irange + 1
    for k, s in enumerate(scores):
        if s > maxv:
            dx, dy, maxv = cx + k % n - irange, cy + k // n - irange, s
    return dx, dy


def register(ref, sec, scaling=False):
    """-> dict: transform (dx, dy, a, b), and per level (0 = full resolution) ref / sec / centre / scores / shift."""
    levels = [(np.asarray(ref, dtype=np.float64), np.asarray(sec, dtype=np.float64))]
    while min(levels[-1][0].shape) > 100:
        levels.append((downsample2x(levels[-1][0]), downsample2x(levels[-1][1])))
    info, cx, cy = [None] * len(levels), 0, 0
    for k in range(len(levels) - 1, -1, -1):
        u, v = levels[k]
        s = ncc_scores(u, v, cx, cy)
        dx, dy = pick(s, cx, cy)
        info[k] = {"ref": u, "sec": v, "centre": (cx, cy), "scores": s, "shift": (dx, dy)}
        cx, cy = 2 * dx, 2 * dy
    dx, dy = info[0]["shift"]
    muu, muv, sigu, sigv, _ = mean_std(levels[0][0], levels[0][1], dx, dy)
    a = sigu / sigv if scaling else 1.0
    return {"transform": (dx, dy, a, muu - muv * a), "levels": info}


# ---------------------------------------------------------------------------------------------------------------- MAE
def mask_water(sec, water):
    out = np.array(sec, dtype=np.float32, copy=True)
    h, w = min(out.shape[0], water.shape[0]), min(out.shape[1], water.shape[1])
    out[:h, :w][np.asarray(water)[:h, :w] != 0] = np.nan
    return out


def dsm_error(gt, sec, transform, water=None):
    """-> (err float32 [h, w], mae float64, n_valid): shift, a*z+b rounded to fp32, clip to the finite GT range +- 10 m, minus GT."""
    gt = np.asarray(gt, dtype=np.float32)
    sec = mask_water(sec, water) if water is not None else np.asarray(sec, dtype=np.float32)
    dx, dy, a, b = transform
    reg = (a * shifted(sec, sec.shape, int(dx), int(dy)) + b).astype(np.float32)
    finite = gt[np.isfinite(gt)]
    lo, hi = (finite.min() - np.float32(10), finite.max() + np.float32(10)) if finite.size else (np.float32(np.inf), np.float32(-np.inf))
    reg = np.where(reg < lo, lo, np.where(reg > hi, hi, reg)).astype(np.float32)
    h, w = min(gt.shape[0], sec.shape[0]), min(gt.shape[1], sec.shape[1])
    err = reg[:h, :w] - gt[:h, :w]
    ok = ~np.isnan(err)
    n = int(ok.sum())
    mae = float(np.abs(err[ok].astype(np.float64)).sum() / n) if n else math.nan
    return err, mae, n
