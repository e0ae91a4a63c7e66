"""TEST INFRASTRUCTURE ONLY -- numpy (fp64) restatement of the true-orthophoto contract of include/eonerf_ortho.h.

Composed of pieces that are pinned elsewhere, so it needs no golden of its own:
  prior_restated.utm_inverse   the arbitrary-precision transverse Mercator (tests/geodesy_exact.py)
  RO.projection                golden g13 (sat_utils.py:420-432)
  ground()                     the arithmetic of get_utmalt_from_nerf_prediction (datasets/satellite.py:514-533)
What is new here -- the pixel convention, the bilinear taps, the weight rules, the two fusion modes -- is checked against an analytic
scene (plane_scene below) in tests/test_ortho_restated_cpu.py: a restatement cannot catch its own sign errors.
"""
import numpy as np

import prior_restated as PR
from oracle import raygen_oracle as RO

MAX_MEDIAN = 64
MEAN, MEDIAN = 0, 1
LON0 = -81.66


# ----------------------------------------------------------------------------- the three contracts
def ground(rays, depth, scene_offset, scene_scale, zone, south=False):
    """eonerf_ortho_ground -> fp64 [n, 3] = lon, lat (degrees), alt; three NaNs for a non-finite depth."""
    rays = np.asarray(rays, dtype=np.float32).astype(np.float64)
    depth = np.asarray(depth, dtype=np.float32).astype(np.float64).reshape(-1)
    off = np.asarray(scene_offset, dtype=np.float32).astype(np.float64)
    sc = np.asarray(scene_scale, dtype=np.float32).astype(np.float64)
    ok = np.isfinite(depth)
    d = np.where(ok, depth, 0.0)
    xyz = (rays[:, 0:3] + rays[:, 3:6] * d[:, None]) * sc + off
    lon, lat = PR.utm_inverse(xyz[:, 0], xyz[:, 1], zone, south)
    out = np.stack([lon, lat, xyz[:, 2]], axis=1)
    out[~ok] = np.nan
    return out


def project(lonlatalt, rpc):
    """(col, row) fp64 [n, 2]: rpc_projection_differentiable on the points."""
    with np.errstate(invalid="ignore"):
        col, row = RO.projection(rpc, lonlatalt[:, 0], lonlatalt[:, 1], lonlatalt[:, 2])
    return np.stack([col, row], axis=1)


def gather(lonlatalt, rpc, pixels, gain, bias, visibility=None, min_visibility=0.2):
    """eonerf_ortho_gather -> (layer fp32 [n, C], weight fp32 [n], colrow fp64 [n, 2])."""
    pixels = np.asarray(pixels, dtype=np.float32)
    h, w, C = pixels.shape
    n = lonlatalt.shape[0]
    colrow = project(lonlatalt, rpc)
    col, row = colrow[:, 0], colrow[:, 1]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lonlatalt).all(axis=1) & (col >= 0) & (col <= w - 1) & (row >= 0) & (row <= h - 1)
    weight = np.ones(n, dtype=np.float32)
    if visibility is not None:
        weight = np.asarray(visibility, dtype=np.float32).copy()
        with np.errstate(invalid="ignore"):
            ok &= weight >= np.float32(min_visibility)
    cs, rs = np.where(ok, col, 0.0), np.where(ok, row, 0.0)
    c0, r0 = np.floor(cs).astype(int), np.floor(rs).astype(int)
    c1, r1 = np.minimum(c0 + 1, w - 1), np.minimum(r0 + 1, h - 1)
    fx, fy = (cs - c0)[:, None], (rs - r0)[:, None]
    p = pixels.astype(np.float64)
    p00, p01, p10, p11 = p[r0, c0], p[r0, c1], p[r1, c0], p[r1, c1]
    ok &= np.isfinite(p00).all(1) & np.isfinite(p01).all(1) & np.isfinite(p10).all(1) & np.isfinite(p11).all(1)
    with np.errstate(invalid="ignore"):
        v = (1 - fy) * ((1 - fx) * p00 + fx * p01) + fy * ((1 - fx) * p10 + fx * p11)
        v = (v - np.asarray(bias, dtype=np.float32).astype(np.float64)) / np.asarray(gain, dtype=np.float32).astype(np.float64)
    weight = np.where(ok, weight, np.float32(0)).astype(np.float32)
    layer = v.astype(np.float32)
    layer[weight == 0] = np.nan
    return layer, weight, colrow


def fuse(layers, weights, mode):
    """eonerf_ortho_fuse -> (mosaic fp32 [n, C], weight_sum fp32 [n], count int32 [n])."""
    layers = np.asarray(layers, dtype=np.float32).astype(np.float64)
    weights = np.asarray(weights, dtype=np.float32).astype(np.float64)
    K, n, C = layers.shape
    with np.errstate(invalid="ignore"):
        use = weights > 0
    count = use.sum(axis=0).astype(np.int32)
    wsum = np.where(use, weights, 0.0).sum(axis=0)
    mosaic = np.full((n, C), np.nan)
    for p in range(n):
        ks = np.nonzero(use[:, p])[0]
        m = len(ks)
        if m == 0:
            continue
        if mode == MEAN:
            acc = np.zeros(C)
            for k in ks:                                        # ascending k
                acc = acc + weights[k, p] * layers[k, p]
            mosaic[p] = acc / wsum[p]
        else:
            s = np.sort(layers[ks, p], axis=0)
            mosaic[p] = 0.5 * (s[(m - 1) // 2] + s[m // 2])
    return mosaic.astype(np.float32), wsum.astype(np.float32), count


def orthorectify(case, mode, depth=None, visibility="case"):
    """The three contracts in a row on a case (or any dict with the same keys) -> dict of every intermediate."""
    vis = case["visibility"] if isinstance(visibility, str) else visibility
    lla = ground(case["rays"], case["depth"] if depth is None else depth, case["scene_offset"], case["scene_scale"], case["zone"], case["south"])
    layers, weights, colrow = [], [], []
    for k, (rpc, img) in enumerate(zip(case["rpcs"], case["images"])):
        lay, wgt, cr = gather(lla, rpc, img, case["gain"][k], case["bias"][k], None if vis is None else vis[k], case["min_visibility"])
        layers.append(lay)
        weights.append(wgt)
        colrow.append(cr)
    layers, weights, colrow = np.stack(layers), np.stack(weights), np.stack(colrow)
    mosaic, wsum, count = fuse(layers, weights, mode)
    return {"lonlatalt": lla, "layers": layers, "weights": weights, "colrow": colrow, "mosaic": mosaic, "weight": wsum, "count": count}


# ----------------------------------------------------------------------------- the fixtures shared by the CPU and the GPU tests
#        name: (seed, lat0, n, K, C, image shapes (h, w) cycled over the K images, point range in normalised x / y, visibility?)
CASES = {
    "tiny": (21, 30.33, 1, 1, 1, [(2, 2)], (-0.7, -0.3, 0.3, 0.7), False),                # the smallest everything
    "block": (22, 30.33, 257, 2, 3, [(12, 9), (9, 12)], (-0.9, 0.9, -0.9, 0.9), True),   # a block tail, an even median
    "odd": (23, 30.33, 33, 3, 4, [(7, 7), (5, 8), (11, 6)], (-0.9, 0.9, -0.9, 0.9), True),
    "cap": (24, 30.33, 64, 64, 3, [(8, 8)], (-0.9, 0.9, -0.9, 0.9), True),                # the K limit of the median
    "edges": (25, 30.33, 48, 3, 2, [(10, 7), (9, 9), (6, 11)], (-1.5, 1.5, -1.5, 1.5), True),
    "south": (26, -30.33, 20, 2, 3, [(6, 5), (5, 6)], (-0.9, 0.9, -0.9, 0.9), True),
}
SCENE_SCALE = (300.0, 300.0, 60.0)       # fp32-representable; 300 m reaches just short of the synthetic RPC's 322 m half footprint
ALT0 = 20.0
MIN_VISIBILITY = 0.2                     # metrics.py:40
# edges: the cells whose inputs are broken by hand
EDGE_NAN_DEPTH, EDGE_INF_DEPTH, EDGE_NAN_VIS, EDGE_UNSEEN = 3, 5, 7, 9


def scene_frame(lat0):
    """(zone, south, fp32 scene offset) around the synthetic RPC's centre."""
    zone, south = RO.utm_zone_number(lat0, LON0), lat0 < 0
    e0, n0 = RO.utm_forward(np.array([lat0]), np.array([LON0]), zone, south)
    return zone, south, np.array([round(float(e0[0])), round(float(n0[0])), ALT0], dtype=np.float32)


def make_case(name):
    """-> dict(rays fp32 [n,11], depth fp32 [n], scene_offset, scene_scale, zone, south, rpcs [K], images [K] of fp32 [h,w,C],
    gain / bias fp32 [K,C], visibility fp32 [K,n] | None, min_visibility).  Image k's RPC is oracle.raygen_oracle.synthetic_rpc(seed + k)
    rescaled so that its 2048 px frame becomes max(h, w) px; the image is the top-left h x w of that frame."""
    seed, lat0, n, K, C, shapes, (xlo, xhi, ylo, yhi), with_vis = CASES[name]
    rng = np.random.default_rng(seed)
    zone, south, offset = scene_frame(lat0)
    rays = np.zeros((n, 11), dtype=np.float32)
    rays[:, 0] = rng.uniform(xlo, xhi, n)
    rays[:, 1] = rng.uniform(ylo, yhi, n)
    rays[:, 2] = 1.0
    d = np.column_stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), -np.ones(n)])
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = 2.2
    depth = rng.uniform(0.9, 1.1, n).astype(np.float32)          # altitudes of ALT0 +- 6 m
    rpcs, images = [], []
    for k in range(K):
        h, w = shapes[k % len(shapes)]
        rpcs.append(RO.rescale_rpc(RO.synthetic_rpc(seed * 100 + k, lat0=lat0, lon0=LON0), max(h, w) / 2048.0))
        images.append(rng.uniform(0.0, 1.0, (h, w, C)).astype(np.float32))
    gain = rng.uniform(0.5, 1.5, (K, C)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, (K, C)).astype(np.float32)
    vis = rng.uniform(0.0, 1.0, (K, n)).astype(np.float32) if with_vis else None
    if name == "edges":
        depth[EDGE_NAN_DEPTH], depth[EDGE_INF_DEPTH] = np.nan, np.inf
        for img in images:
            img[rng.random(img.shape[:2]) < 0.15] = np.nan         # NaN pixels under some taps
        vis[0, EDGE_NAN_VIS] = np.nan
        vis[:, EDGE_UNSEEN] = 0.05                                   # below min_visibility in every image
        rays[EDGE_UNSEEN, 0:2] = 0.1                                 # ... though it projects inside all of them
    return {"rays": rays, "depth": depth, "scene_offset": offset, "scene_scale": np.array(SCENE_SCALE, dtype=np.float32), "zone": zone,
            "south": south, "rpcs": rpcs, "images": images, "gain": gain, "bias": bias, "visibility": vis, "min_visibility": MIN_VISIBILITY}


def tie_margin(case, res, tol=1e-6):
    """The smallest distance of any projected coordinate from 0, w - 1, h - 1, and of any visibility from min_visibility: above `tol`
    the weight-zero cells of two correct implementations are the same cells."""
    worst = np.inf
    for k, img in enumerate(case["images"]):
        h, w = img.shape[:2]
        cr = res["colrow"][k]
        cr = cr[np.isfinite(cr).all(axis=1)]
        for v, hi in ((cr[:, 0], w - 1), (cr[:, 1], h - 1)):
            worst = min(worst, np.abs(v).min(), np.abs(v - hi).min())
    if case["visibility"] is not None:
        v = case["visibility"][np.isfinite(case["visibility"])].astype(np.float64)
        worst = min(worst, np.abs(v - float(np.float32(case["min_visibility"]))).min())
    return worst


# ----------------------------------------------------------------------------- the analytic scene of the convention test
PLANE_S, PLANE_ALT, PLANE_GRID = 64, 25.0, 16
PLANE_GE, PLANE_GN = 7.5e-4, -5.0e-4       # per metre: f spans about 0.1 .. 0.9 over the 644 m footprint


def plane_scene():
    """A plane at altitude PLANE_ALT carrying the pattern f(E, N) = 0.5 + gE (E - E0) + gN (N - N0), seen by two synthetic images of
    PLANE_S px (each pixel (c, r) holds f at utm_forward(RO.localization(rpc, c, r, alt))), and a 16 x 16 grid of vertical rays that
    meet the plane at depth 1 inside both footprints.  -> a case dict plus "truth" (f at the points, fp64 [n]) and "bound":
    one tenth of the largest change of f across one pixel, 0.1 * gsd * (|gE| + |gN|).  A swap of row and col, a flip of north or
    a half-pixel shift errs by at least five times that; the RPC's curvature is orders of magnitude below it."""
    lat0 = 30.33
    zone, south, offset = scene_frame(lat0)
    offset[2] = PLANE_ALT
    scale = np.array([250.0, 250.0, 50.0], dtype=np.float32)
    E0, N0 = float(offset[0]), float(offset[1])

    def f(E, N):
        return 0.5 + PLANE_GE * (E - E0) + PLANE_GN * (N - N0)
    rpcs, images = [], []
    cols, rows = np.meshgrid(np.arange(PLANE_S), np.arange(PLANE_S))
    for seed in (1, 2):
        rpc = RO.rescale_rpc(RO.synthetic_rpc(seed, lat0=lat0, lon0=LON0), PLANE_S / 2048.0)
        lon, lat = RO.localization(rpc, cols.ravel().astype(np.float64), rows.ravel().astype(np.float64), np.full(cols.size, PLANE_ALT))
        E, N = RO.utm_forward(lat, lon, zone, south)
        rpcs.append(rpc)
        images.append(f(E, N).reshape(PLANE_S, PLANE_S, 1).astype(np.float32))
    g = np.linspace(-0.8, 0.8, PLANE_GRID).astype(np.float32)
    X, Y = np.meshgrid(g, g[::-1])                              # row 0 is the northern edge, as in a nadir grid
    n = X.size
    rays = np.zeros((n, 11), dtype=np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5], rays[:, 7] = X.ravel(), Y.ravel(), 1.0, -1.0, 2.2
    depth = np.ones(n, dtype=np.float32)                        # z_n = 0: the plane
    truth = f(rays[:, 0].astype(np.float64) * float(scale[0]) + E0, rays[:, 1].astype(np.float64) * float(scale[1]) + N0)
    gsd = 0.3 * 2048.0 / PLANE_S * (1.1 / 1.05)                 # metres per pixel of the rescaled frame (prior_restated.make_case)
    return {"rays": rays, "depth": depth, "scene_offset": offset, "scene_scale": scale, "zone": zone, "south": south, "rpcs": rpcs,
            "images": images, "gain": np.ones((2, 1), dtype=np.float32), "bias": np.zeros((2, 1), dtype=np.float32), "visibility": None,
            "min_visibility": MIN_VISIBILITY, "truth": truth, "bound": 0.1 * gsd * (abs(PLANE_GE) + abs(PLANE_GN))}
