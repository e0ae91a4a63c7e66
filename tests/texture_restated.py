"""TEST INFRASTRUCTURE ONLY -- numpy (fp64) restatement of the texture contract of eonerf_code_amd/csrc/eonerf_texture.h: the atlas
layout, texel ownership, UVs, clamped barycentric weights, the samples and the fused bake.

The shared expressions are not restated twice: the projection, the bilinear gather and the two fusion modes are
ortho_restated.project / gather / fuse, the inverse UTM is prior_restated.utm_inverse.  What is new here -- the layout rule, the
clamp, the incidence weight, BEST -- is checked against analytic scenes in tests/test_texture_restated_cpu.py.
"""
import math

import numpy as np

import ortho_restated as OR
import prior_restated as PR

VERSION = 1
MAX_TEXELS = 64
GUTTER = 5
MAX_SIDE = 32768
MAX_MEDIAN = 64
MEAN, MEDIAN, BEST = 0, 1, 2


# ----------------------------------------------------------------------------- the atlas
def layout(n_faces, texels):
    """(atlas_w, atlas_h, cells_per_row, cells), or None where eonerf_texture_layout answers EONERF_E_UNSUPPORTED."""
    assert n_faces >= 0 and 1 <= texels <= MAX_TEXELS
    S = texels + GUTTER
    cells = (n_faces + 1) // 2
    cpr = math.isqrt(cells)
    if cpr * cpr < cells:
        cpr += 1
    rows = -(-cells // cpr) if cpr else 0
    w, h = cpr * S, rows * S
    if w > MAX_SIDE or h > MAX_SIDE or w * h > (1 << 31) - 1:
        return None
    return w, h, cpr, cells


def corners(n_faces, texels):
    """fp64 [F, 3, 2]: the atlas position (u, v), in texels from the top left, of the corners A, B, C of every face."""
    w, h, cpr, cells = layout(n_faces, texels)
    S = texels + GUTTER
    f = np.arange(n_faces, dtype=np.int64)
    j = f // 2
    lower = f % 2 == 0
    a = np.where(lower, 1.5, S - 1.5)
    leg = np.where(lower, float(texels), -float(texels))
    u0, v0 = (j % max(cpr, 1) * S).astype(np.float64), (j // max(cpr, 1) * S).astype(np.float64)
    out = np.empty((n_faces, 3, 2))
    out[:, :, 0] = (u0 + a)[:, None]
    out[:, :, 1] = (v0 + a)[:, None]
    out[:, 1, 0] = u0 + (a + leg)
    out[:, 2, 1] = v0 + (a + leg)
    return out


def uv(n_faces, texels):
    """eonerf_texture_uv -> fp32 [F, 3, 2] = (u / atlas_w, 1 - v / atlas_h)."""
    w, h, _, _ = layout(n_faces, texels)
    c = corners(n_faces, texels)
    if n_faces == 0:
        return np.zeros((0, 3, 2), dtype=np.float32)
    return np.stack([c[..., 0] / float(w), 1.0 - c[..., 1] / float(h)], axis=-1).astype(np.float32)


def texels_of(n_faces, texels, first=0, n=None):
    """Ownership and clamped weights of the texels [first, first + n): (face int32 [n], bary fp64 [n, 3]); -1 and NaN for a texel no
    face owns."""
    w, h, cpr, cells = layout(n_faces, texels)
    n = w * h - first if n is None else n
    assert first >= 0 and n >= 0 and first + n <= w * h
    S = texels + GUTTER
    t = first + np.arange(n, dtype=np.int64)
    x, y = t % max(w, 1), t // max(w, 1)
    cx, cy = x % S, y % S
    j = (y // S) * cpr + x // S
    lower = cx + cy <= S - 1
    face = 2 * j + np.where(lower, 0, 1)
    owned = (j < cells) & (face < n_faces)
    u, v = cx + 0.5, cy + 0.5
    ua = np.where(lower, 1.5, S - 1.5)
    leg = np.where(lower, float(texels), -float(texels))
    b1, b2 = (u - ua) / leg, (v - ua) / leg
    b0 = (1.0 - b1) - b2
    b = np.maximum(np.stack([b0, b1, b2], axis=1), 0.0)
    b = b / ((b[:, 0] + b[:, 1]) + b[:, 2])[:, None]
    b[~owned] = np.nan
    return np.where(owned, face, -1).astype(np.int32), b


def samples(vertices, triangles, texels, scene_offset, scene_scale, zone, south, first=0, n=None):
    """eonerf_texture_samples -> dict(face int32 [n], bary fp32 [n, 3], xyz fp32 [n, 3], xyz64, lonlatalt fp64 [n, 3], normal fp32 [n, 3],
    normal64)."""
    V = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3).astype(np.int64)
    off = np.asarray(scene_offset, dtype=np.float32).astype(np.float64)
    sc = np.asarray(scene_scale, dtype=np.float32).astype(np.float64)
    F = tri.shape[0]
    face, b = texels_of(F, texels, first, n)
    n = face.shape[0]
    f = np.maximum(face, 0).astype(np.int64)
    idx = tri[f] if F else np.zeros((n, 3), dtype=np.int64)
    inside = ((idx >= 0) & (idx < V.shape[0])).all(axis=1) & (face >= 0)
    idx = np.where(inside[:, None], idx, 0)
    Vs = V if V.shape[0] else np.zeros((1, 3))
    A, B, C = Vs[idx[:, 0]], Vs[idx[:, 1]], Vs[idx[:, 2]]
    ok = inside & np.isfinite(A).all(1) & np.isfinite(B).all(1) & np.isfinite(C).all(1)
    A, B, C = (np.where(ok[:, None], P, 0.0) for P in (A, B, C))
    with np.errstate(invalid="ignore", divide="ignore"):
        bb = np.where(ok[:, None], b, 0.0)
        p = (bb[:, 0:1] * A + bb[:, 1:2] * B) + bb[:, 2:3] * C
        e1, e2 = (B - A) * sc, (C - A) * sc
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = ok & (length > 0) & np.isfinite(length)
        nrm = np.stack([nx, ny, nz], axis=1) / np.where(good, length, 1.0)[:, None]
    nrm[~good] = np.nan
    p[~ok] = np.nan
    m = np.where(ok[:, None], p, 0.0) * sc + off
    lon, lat = PR.utm_inverse(m[:, 0], m[:, 1], zone, south)
    lla = np.stack([lon, lat, m[:, 2]], axis=1)
    lla[~ok] = np.nan
    return {"face": face, "bary": b.astype(np.float32), "xyz": p.astype(np.float32), "xyz64": p, "lonlatalt": lla,
            "normal": nrm.astype(np.float32), "normal64": nrm}


# ----------------------------------------------------------------------------- the bake
def image_weights(normal, to_satellite, gain, bias, blocked, min_cos, angle_weight, n):
    """What eonerf_texture_bake decides before it projects: (w fp32 [K, n]: 0, 1 or (float) cos;  cos fp64 [K, n] | None)."""
    gain, bias = np.asarray(gain, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    K = gain.shape[0]
    w = np.ones((K, n), dtype=np.float32)
    good = (np.isfinite(gain) & (gain != 0) & np.isfinite(bias)).all(axis=1)
    w[~good] = 0
    if blocked is not None:
        w[np.asarray(blocked).reshape(K, n) != 0] = 0
    cos = None
    if normal is not None:
        nr = np.asarray(normal, dtype=np.float32).astype(np.float64)
        s = np.asarray(to_satellite, dtype=np.float64).reshape(K, 3)
        with np.errstate(invalid="ignore"):
            cos = (nr[None, :, 0] * s[:, None, 0] + nr[None, :, 1] * s[:, None, 1]) + nr[None, :, 2] * s[:, None, 2]
            keep = cos >= float(np.float32(min_cos))
            if angle_weight:
                w = np.where(w > 0, cos.astype(np.float32), w)
            w = np.where(keep, w, np.float32(0)).astype(np.float32)
    return w, cos


def bake(lonlatalt, normal, rpcs, images, gain, bias, to_satellite=None, blocked=None, min_cos=0.1, angle_weight=True, mode=MEDIAN,
         return_all=False):
    """eonerf_texture_bake -> dict(colour fp32 [n, C], weight fp32 [n], count int32 [n], best int32 [n])."""
    lla = np.asarray(lonlatalt, dtype=np.float64)
    n, K = lla.shape[0], len(images)
    gain, bias = np.asarray(gain, dtype=np.float32), np.asarray(bias, dtype=np.float32)
    pre, cos = image_weights(normal, to_satellite, gain, bias, blocked, min_cos, angle_weight, n)
    layers, weights, colrow = [], [], []
    for k in range(K):
        usable = bool((np.isfinite(gain[k]) & (gain[k] != 0) & np.isfinite(bias[k])).all())
        g, b = (gain[k], bias[k]) if usable else (np.ones_like(gain[k]), np.zeros_like(bias[k]))
        lay, wgt, cr = OR.gather(lla, rpcs[k], images[k], g, b)
        with np.errstate(invalid="ignore"):
            wk = np.where((wgt > 0) & (pre[k] > 0), pre[k], np.float32(0)).astype(np.float32)
        lay = lay.copy()
        lay[wk == 0] = np.nan
        layers.append(lay)
        weights.append(wk)
        colrow.append(cr)
    layers, weights = np.stack(layers), np.stack(weights)
    count = (weights > 0).sum(axis=0).astype(np.int32)
    best = np.where(count > 0, np.argmax(weights, axis=0), -1).astype(np.int32)         # argmax: the first of equal maxima
    if mode == BEST:
        wsum = np.where(weights > 0, weights.astype(np.float64), 0.0).sum(axis=0).astype(np.float32)
        colour = np.where((count > 0)[:, None], layers[np.maximum(best, 0), np.arange(n)], np.float32(np.nan)).astype(np.float32)
    else:
        colour, wsum, cnt = OR.fuse(layers, weights, mode)
        assert (cnt == count).all()
    out = {"colour": colour, "weight": wsum, "count": count, "best": best}
    if return_all:
        out.update(layers=layers, weights=weights, colrow=np.stack(colrow), cos=cos)
    return out


def to_satellite(view_dirs, scene_scale):
    """fp64 [K, 3]: normalised-scene view directions (satellite -> ground) scaled into the metric frame, negated and normalised."""
    d = np.asarray(view_dirs, dtype=np.float32).astype(np.float64) * np.asarray(scene_scale, dtype=np.float32).astype(np.float64)
    d = -d
    return d / np.sqrt((d * d).sum(axis=1, keepdims=True))


# ----------------------------------------------------------------------------- bilinear lookup of an atlas, as a viewer does it
def bilinear_taps(u, v, w, h):
    """The four taps of a bilinear lookup at the atlas position (u, v) in texels (texel centres at half-integers): [(x, y, weight)],
    not clamped to the atlas -- a tap of non-zero weight outside it is the caller's finding."""
    fx, fy = u - 0.5, v - 0.5
    x0, y0 = math.floor(fx), math.floor(fy)
    ax, ay = fx - x0, fy - y0
    taps = []
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            taps.append((x0 + dx, y0 + dy, wx * wy))
    return taps
