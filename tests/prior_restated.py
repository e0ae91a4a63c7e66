"""TEST INFRASTRUCTURE ONLY -- numpy (fp64) restatement of the depth-prior contract of include/eonerf_prior.h.

Follows sat_utils.py:310-362,420-432 (reproject_dsm_alt_to_satellite_image, the RPC projection) and datasets/satellite.py:644-653,
677-679 (altitude -> depth, NaN -> -1) of the reference.  Golden g13 (tests/golden/make_golden_prior.py) pins everything here to
the reference's own code except utm_inverse.

PARITY STATUS of utm_inverse: pinned by a definition-based arbitrary-precision transverse Mercator (tests/geodesy_exact.py,
tests/test_geodesy_exact_cpu.py: within 1e-12 degrees, measured 1.4e-14), like utm_forward of oracle/raygen_oracle.py.  pyproj / PROJ
themselves are absent from the reference tree and from this image.  It is restated from the algorithm PROJ's etmerc implements (Karney 2011): the 6th-order Krueger series with
the beta coefficients (eq. 36), then Newton on tau = tan(lat) from the conformal latitude (eqs. 19-21), a fixed five iterations.
In-tree anchor: utm_forward(utm_inverse(e, n)) == (e, n) to 1e-6 m (tests/test_prior_restated_cpu.py).
"""
import math

import numpy as np

from oracle import raygen_oracle as RO

KRUEGER_NEWTON = 5
R2D = 57.29577951308232


def krueger_beta():
    n = RO.WGS84_F / (2.0 - RO.WGS84_F)
    n2 = n * n
    n3 = n2 * n
    n4 = n3 * n
    n5 = n4 * n
    n6 = n5 * n
    return [n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
            n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
            17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
            4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
            4583 * n5 / 161280 - 108847 * n6 / 3991680,
            20648693 * n6 / 638668800]


def utm_inverse(easts, norths, zone, south=False):
    """(lon, lat) in degrees of "+proj=utm +zone=<zone> [+south]" -> "+proj=latlon" on WGS84."""
    A, _, e = RO.krueger_alpha()
    k0A = RO.UTM_K0 * A
    xi = (np.asarray(norths, dtype=np.float64) - (10000000.0 if south else 0.0)) / k0A
    eta = (np.asarray(easts, dtype=np.float64) - 500000.0) / k0A
    xi_p, eta_p = xi.copy(), eta.copy()
    for j, bj in enumerate(krueger_beta(), start=1):
        xi_p = xi_p - bj * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        eta_p = eta_p - bj * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    sh, c = np.sinh(eta_p), np.cos(xi_p)
    lam = np.arctan2(sh, c)
    taup = np.sin(xi_p) / np.sqrt(sh * sh + c * c)
    e2m = 1.0 - e * e
    tau = taup / e2m
    for _ in range(KRUEGER_NEWTON):
        tau1 = np.sqrt(1.0 + tau * tau)
        sig = np.sinh(e * np.arctanh(e * tau / tau1))
        taupa = np.sqrt(1.0 + sig * sig) * tau - sig * tau1
        tau = tau + (taup - taupa) * (1.0 + e2m * tau * tau) / (e2m * tau1 * np.sqrt(1.0 + taupa * taupa))
    return (zone * 6.0 - 183.0) + lam * R2D, np.arctan(tau) * R2D


def sample_points(h, w, bounds):
    """sat_utils.py:318-333: (easts, norths, index1d) of the (2h) x (2w) sample grid, raveled.  bounds = left, bottom, right, top."""
    left, bottom, right, top = (float(b) for b in bounds)
    x_min, x_max, y_min, y_max = min(left, right), max(left, right), min(bottom, top), max(bottom, top)
    X, Y = np.meshgrid(np.linspace(x_min, x_max, w * 2), np.linspace(y_max, y_min, h * 2))
    dsm_cols, dsm_rows = np.meshgrid(np.linspace(0, w - 1, w * 2), np.linspace(0, h - 1, h * 2))
    dsm_cols, dsm_rows = dsm_cols.astype(int).ravel(), dsm_rows.astype(int).ravel()
    return X.ravel(), Y.ravel(), (dsm_rows * w + dsm_cols).astype(int)


def reproject(dsm, bounds, rpc, out_h, out_w, zone, south=False, values=None, full=False):
    """reproject_dsm_alt_to_satellite_image -> fp32 [out_h, out_w] (NaN = empty).  full: a dict with the intermediates as well:
    cols / rows (fp64, every sample point), winner (uint32 [out_h, out_w]: 1 + raveled index of the point a pixel keeps, 0 = none),
    index1d, lon, lat."""
    dsm = np.asarray(dsm, dtype=np.float32)
    h, w = dsm.shape
    easts, norths, index1d = sample_points(h, w, bounds)
    alts = dsm.ravel()[index1d]
    lons, lats = utm_inverse(easts, norths, zone, south)
    with np.errstate(invalid="ignore"):
        cols, rows = RO.projection(rpc, lons, lats, alts.astype(np.float64))
        valid = (cols >= 0) & (cols < out_w) & (rows >= 0) & (rows < out_h)
    src = np.asarray(values, dtype=np.float32).ravel() if values is not None else dsm.ravel()
    out = np.full((out_h, out_w), np.nan, dtype=np.float32)
    r, c = rows[valid].astype(np.int16), cols[valid].astype(np.int16)
    out[r, c] = src[index1d][valid]                                   # the last point in raveled order wins
    if not full:
        return out
    winner = np.zeros((out_h, out_w), dtype=np.uint32)
    np.maximum.at(winner, (r.astype(int), c.astype(int)), (np.nonzero(valid)[0] + 1).astype(np.uint32))
    return {"raster": out, "cols": cols, "rows": rows, "valid": valid, "winner": winner, "index1d": index1d, "lon": lons, "lat": lats,
            "easts": easts, "norths": norths}


def depth_prior(alt_raster, rays, z_offset, z_scale):
    """datasets/satellite.py:646-653 and the cast of :701: fp32 [h*w] depth along each pixel's ray, -1 where there is no altitude."""
    alts = np.asarray(alt_raster, dtype=np.float32).ravel().astype(np.float64)
    rays = np.asarray(rays, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (alts - float(np.float32(z_offset))) / float(np.float32(z_scale))
        depth = (a - rays[:, 2]) / rays[:, 5]
    depth[np.isnan(depth)] = -1.0
    return depth.astype(np.float32)


def conf_prior(conf_raster):
    """datasets/satellite.py:678-679."""
    c = np.asarray(conf_raster, dtype=np.float32).ravel().copy()
    c[np.isnan(c)] = -1.0
    return c


def ambiguous_pixels(cols, rows, out_h, out_w, tol=1e-9):
    """bool [out_h, out_w]: pixels a sample point could enter or leave under a perturbation of `tol` px of its fp64 col / row, i.e.
    the point lies within tol of an integer (image edges are integers).  Device and numpy sin / atanh differ by an ulp (~1e-12 px), so
    only these pixels may legitimately differ between two correct implementations."""
    bad = np.zeros((out_h, out_w), dtype=bool)
    ok = np.isfinite(cols) & np.isfinite(rows)
    c, r = cols[ok], rows[ok]
    near = (np.abs(c - np.round(c)) < tol) | (np.abs(r - np.round(r)) < tol)
    for cc, rr in zip(c[near], r[near]):
        for dc in (-tol, tol):
            for dr in (-tol, tol):
                i, j = math.floor(rr + dr), math.floor(cc + dc)
                if 0 <= i < out_h and 0 <= j < out_w:
                    bad[i, j] = True
    return bad


# ----------------------------------------------------------------------------- the fixtures shared by the golden recipe and the tests
def terrain(rng, h, w, nan_block=None):
    """Smooth relief + a little roughness, in 1/64 m steps (float32-representable)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z = 22 + 9 * np.sin(xx / max(w, 2) * 5.1) * np.cos(yy / max(h, 2) * 3.7) + rng.uniform(-1.5, 1.5, (h, w))
    z = (np.round(z * 64) / 64).astype(np.float32)
    if nan_block is not None:
        r0, r1, c0, c1 = nan_block
        z[r0:r1, c0:c1] = np.nan
    return z


#        name: (seed, lat0, DSM h x w, image h x w, DSM centre (row, col) px, DSM extent (rows, cols) px, NaN block, confidence?)
CASES = {
    "tiny": (3, 30.33, (9, 7), (12, 10), (6.0, 5.0), (11.0, 9.0), None, False),
    "outside": (5, 30.33, (64, 48), (40, 56), (34.0, 40.0), (45.0, 50.0), (10, 20, 5, 15), False),      # sticks out right and below
    "collide": (7, 30.33, (128, 128), (16, 16), (8.0, 8.0), (14.0, 14.0), None, False),               # 65,536 points onto 256 pixels
    "south": (9, -30.33, (11, 13), (14, 9), (7.0, 4.0), (12.0, 10.0), (2, 4, 3, 6), False),
    "conf": (11, 30.33, (24, 18), (20, 28), (12.0, 16.0), (22.0, 30.0), (4, 9, 2, 7), True),
}
GOLDEN_CASES = ("tiny", "south", "conf")      # what fits the fixture's size limit with the lon / lat of every sample point


def make_case(name):
    """-> dict(dsm, values | None, bounds, rpc, out_h, out_w, zone, south).  The RPC is oracle.raygen_oracle.synthetic_rpc rescaled so
    that its 2048 px frame becomes max(out_h, out_w) px; the image is the top-left out_h x out_w of that frame."""
    seed, lat0, (h, w), (out_h, out_w), (cr, cc), (er, ec), nan_block, with_conf = CASES[name]
    lon0 = -81.66
    S = max(out_h, out_w)
    rpc = RO.rescale_rpc(RO.synthetic_rpc(seed, lat0=lat0, lon0=lon0), S / 2048.0)
    zone, south = RO.utm_zone_number(lat0, lon0), lat0 < 0
    e0, n0 = RO.utm_forward(np.array([lat0]), np.array([lon0]), zone, south)
    gsd = 0.3 * 2048.0 / S * (1.1 / 1.05)                       # metres per pixel of the rescaled frame, roughly
    ce, cn = float(e0[0]) + (cc - S / 2.0) * gsd, float(n0[0]) - (cr - S / 2.0) * gsd
    q = lambda v: round(v * 4) / 4                              # noqa: E731 -- bounds on a 0.25 m lattice
    bounds = [q(ce - ec * gsd / 2), q(cn - er * gsd / 2), q(ce + ec * gsd / 2), q(cn + er * gsd / 2)]
    rng = np.random.default_rng(seed)
    dsm = terrain(rng, h, w, nan_block)
    values = None
    if with_conf:
        values = rng.integers(0, 8, (h, w)).astype(np.float32)
        values[rng.random((h, w)) < 0.05] = np.nan
    return {"dsm": dsm, "values": values, "bounds": bounds, "rpc": rpc, "out_h": out_h, "out_w": out_w, "zone": zone, "south": south}


def case_rays(case, seed=0):
    """fp32 [out_h*out_w, 11] stand-in rays for the depth arithmetic (only o_z and d_z matter): origins near z = 1, steep directions."""
    rng = np.random.default_rng(1000 + seed)
    n = case["out_h"] * case["out_w"]
    rays = np.zeros((n, 11), dtype=np.float32)
    rays[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    rays[:, 2] = rng.uniform(0.9, 1.0, n)
    d = np.column_stack([rng.normal(0, 0.2, n), rng.normal(0, 0.2, n), -np.ones(n)])
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = 2.2
    return rays


Z_OFFSET, Z_SCALE = 20.0, 61.5       # scene Z offset / scale of the depth cases (fp32-representable)
