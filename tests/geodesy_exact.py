"""TEST INFRASTRUCTURE ONLY -- transverse Mercator on WGS84 straight from its definition, in arbitrary precision (mpmath), with no
series: the yardstick for the two Krueger-series restatements (oracle/raygen_oracle.utm_forward, tests/prior_restated.utm_inverse) and
the two device routines behind them (k_raygen, k_prior_splat).  It shares no coefficient with any of them.

Definition (Gauss-Krueger; e.g. Karney 2011, section 2).  With e the first eccentricity,
    isometric latitude   psi(phi) = atanh(sin phi) - e atanh(e sin phi)
    meridian arc         S(phi)   = a (1 - e^2) * integral_0^phi (1 - e^2 sin^2 t)^(-3/2) dt
both continued analytically to complex phi.  The projection is the conformal map that is true to scale k0 on the central meridian:
    psi(Phi) = psi(phi) + i lambda        (lambda = longitude - central meridian; solved for the complex latitude Phi)
    north + i east = k0 S(Phi)            (+ the false origin: 500 000 m east, 10 000 000 m north with "+south")
The integrand's branch points sit at sin t = +-1/e (|Im t| ~ 3.2), far from any path used here (|Im Phi| < 0.12 at 6 degrees off).

mpmath comes with torch (torch -> sympy -> mpmath).  Inputs are taken as the exact binary values of the fp64 arguments; everything
runs at DIGITS significant digits; the outputs are rounded to fp64 once.  Results are memoised per process on the argument tuple, so
the CPU and the GPU tests that share points pay once (~8 ms per forward point, ~50 ms per inverse point)."""
import functools

import mpmath as mp

DIGITS = 40
A = 6378137
INV_F = "298.257223563"
K0 = "0.9996"
FALSE_EAST = 500000
FALSE_NORTH_SOUTH = 10000000


def central_meridian(zone):
    return 6 * int(zone) - 183


class _Ctx:
    """The constants at DIGITS digits (built inside the precision context, once)."""
    def __init__(self):
        self.f = 1 / mp.mpf(INV_F)
        self.e2 = self.f * (2 - self.f)
        self.e = mp.sqrt(self.e2)
        self.a = mp.mpf(A)
        self.k0 = mp.mpf(K0)
        self.d2r = mp.pi / 180


@functools.lru_cache(maxsize=None)
def _c():
    with mp.workdps(DIGITS):
        return _Ctx()


def psi(phi):
    """Isometric latitude, complex phi allowed."""
    c = _c()
    s = mp.sin(phi)
    return mp.atanh(s) - c.e * mp.atanh(c.e * s)


def dpsi(phi):
    c = _c()
    return (1 - c.e2) / ((1 - c.e2 * mp.sin(phi) ** 2) * mp.cos(phi))


def _w(phi):
    c = _c()
    return (1 - c.e2 * mp.sin(phi) ** 2) ** mp.mpf(-1.5)


def dS(phi):
    c = _c()
    return c.a * (1 - c.e2) * _w(phi)


def S(phi):
    """Meridian arc from the equator to phi, along the straight segment 0 -> phi (phi complex allowed).  The integrand handed to
    mp.quad is O(1): quad judges its error absolutely, against the working precision plus a few guard bits."""
    c = _c()
    phi = mp.mpmathify(phi)
    return c.a * (1 - c.e2) * phi * mp.quad(lambda u: _w(u * phi), [0, 1], method="gauss-legendre")            # t = u phi, dt = phi du


def _newton(f, df, x, ladder=True):
    """Root of the analytic f from a start good to ~1e-2.  Quadratic convergence: five steps at 15 digits reach their round-off, two at
    DIGITS square 1e-15 twice.  ladder=False runs seven steps at DIGITS (1e-2 -> 1e-64 after six): mp.quad judges its error
    absolutely, which a short working precision never satisfies, so the steps through S are cheapest at full precision."""
    if ladder:
        with mp.workdps(15):
            for _ in range(5):
                x = x - f(x) / df(x)
    for _ in range(2 if ladder else 7):
        x = x - f(x) / df(x)
    return x


def _forward_mp(lat, lon, zone):
    """-> (east - 500000, north) unrounded, without the false northing."""
    c = _c()
    phi = mp.mpf(float(lat)) * c.d2r
    lam = (mp.mpf(float(lon)) - central_meridian(zone)) * c.d2r
    target = psi(phi) + mp.mpc(0, lam)
    Phi = _newton(lambda z: psi(z) - target, dpsi, mp.mpc(phi, lam * mp.cos(phi)))
    z = c.k0 * S(Phi)
    return mp.im(z), mp.re(z)


@functools.lru_cache(maxsize=None)
def _forward_cached(lat, lon, zone):
    with mp.workdps(DIGITS):
        return _forward_mp(lat, lon, zone)


def forward_mp(lat, lon, zone, south=False):
    """(east, north) as mpmath numbers at DIGITS digits.  `south` is the projection's "+south" flag, not the sign of the latitude."""
    x, y = _forward_cached(float(lat), float(lon), int(zone))
    with mp.workdps(DIGITS):
        return x + FALSE_EAST, y + (FALSE_NORTH_SOUTH if south else 0)


def forward(lat, lon, zone, south=False):
    """(east, north) in metres, fp64 (rounded once)."""
    e, n = forward_mp(lat, lon, zone, south)
    return float(e), float(n)


def _inverse_mp(east, north, zone, south):
    """east / north: floats or mpmath numbers (the helper's self-check feeds the unrounded forward image); call inside workdps."""
    c = _c()
    z = mp.mpc(mp.mpf(north) - (FALSE_NORTH_SOUTH if south else 0), mp.mpf(east) - FALSE_EAST) / c.k0
    Phi = _newton(lambda p: S(p) - z, dS, z / c.a, ladder=False)
    w = psi(Phi)
    lam = mp.im(w)
    q = mp.re(w)
    phi = _newton(lambda p: psi(p) - q, dpsi, mp.re(Phi))
    return central_meridian(zone) + lam / c.d2r, phi / c.d2r


@functools.lru_cache(maxsize=None)
def _inverse_cached(east, north, zone, south):
    with mp.workdps(DIGITS):
        return _inverse_mp(east, north, zone, south)


def inverse_mp(east, north, zone, south=False):
    """(lon, lat) in degrees as mpmath numbers at DIGITS digits."""
    return _inverse_cached(float(east), float(north), int(zone), bool(south))


def inverse(east, north, zone, south=False):
    """(lon, lat) in degrees, fp64 (rounded once)."""
    lon, lat = inverse_mp(east, north, zone, south)
    return float(lon), float(lat)


# ----------------------------------------------------------------------------- the shared point list (CPU and GPU tests)
ZONES = (1, 17, 31, 32, 34, 60)
LATS = (1e-9, -1e-9, 0.001, -0.001, 30.33, -30.33, 45.0, -45.0, 60.0, -60.0, 79.9, -79.9, 84.0)
DLONS = (0.0, 1e-6, -1e-6, 1.0, -1.0, 3.0, -3.0, 3.5, -3.5)


def point_list():
    """[(lat, lon, zone, south)]: every zone of ZONES meets every latitude of LATS, each at two of the longitude offsets DLONS (taken
    in rotation, so every offset meets every zone and both hemispheres): 6 x 13 x 2 = 156 points with south = (lat < 0).  Then Norway's
    widened zone 32 at 3 E, 60 N -- six degrees off its meridian -- and two points whose "+south" contradicts their latitude."""
    pts, k = [], 0
    for zone in ZONES:
        lon0 = float(central_meridian(zone))
        for lat in LATS:
            for _ in range(2):
                pts.append((lat, lon0 + DLONS[k % len(DLONS)], zone, lat < 0))
                k += 2                                  # 9 offsets, stride 2: all nine come round
            k += 1
    pts.append((60.0, 3.0, 32, False))
    pts.append((30.33, -81.66, 17, True))
    pts.append((-33.9, 18.4, 34, False))
    return pts


NORWAY = (60.0, 3.0, 32, False)


# ----------------------------------------------------------------------------- the magnifier fixtures of the inverse (CPU and GPU tests)
# k_prior_splat shows no lon / lat, only the pixel a DSM sample point lands in -- so the pixel is made tiny.  An identity RPC centred on a
# point P (col <- longitude, row <- latitude) with one pixel = MAG_PIXEL_DEG degrees (11 um of latitude) over a MAG_SIZE^2 image, and a
# 2 x 2 DSM of altitude 0 whose 4 x 4 sample points straddle P's exact forward image.  The DSM spans 3 cm of northing and 3 cm x cos(lat)
# of easting: ~2700 px each way at every latitude (a full 3 cm of easting is 5400 px at 60 N and 15 000 px at 79.9 N, outside the image).
MAG_PIXEL_DEG = 1e-10
MAG_SIZE = 4096
#              name: (lat, lon, zone, south[, (dcol, drow)]): the DSM is centred (dcol, drow) px beside P where the centred one would put a
#              sample point within 1e-3 px of a pixel edge (tests/test_geodesy_exact_cpu.py checks every case)
MAGNIFIER = {
    "jacksonville": (30.33, -81.66, 17, False, (2.3, 3.7)),
    "zone17_edge": (30.33, -78.01, 17, False),           # 2.99 degrees off the meridian
    "cape_town": (-33.9, 18.4, 34, True),
    "equator_north": (1e-4, -81.66, 17, False),
    "equator_south": (-1e-4, 18.4, 34, True),
    "arctic": (79.9, 1.5, 31, False),
    "norway": (60.0, 5.0, 32, False),                    # the widened zone 32: 4 degrees off its meridian
    "antimeridian": (40.0, 179.9, 60, False),
}


def magnifier_case(name):
    """-> dict(dsm, bounds, rpc, out_h, out_w, zone, south) in the shape of prior_restated.make_case."""
    import math
    import numpy as np
    lat, lon, zone, south = MAGNIFIER[name][:4]
    dcol, drow = MAGNIFIER[name][4] if len(MAGNIFIER[name]) > 4 else (0.0, 0.0)
    half = MAG_SIZE / 2.0
    rpc = {"row_offset": half, "col_offset": half, "row_scale": half, "col_scale": half, "lat_offset": lat, "lon_offset": lon,
           "alt_offset": 0.0, "lat_scale": MAG_PIXEL_DEG * half, "lon_scale": MAG_PIXEL_DEG * half, "alt_scale": 1.0,
           "col_num": [0.0, 1.0] + [0.0] * 18, "row_num": [0.0, 0.0, 1.0] + [0.0] * 17,      # apply_poly: [1] x lon, [2] x lat
           "col_den": [1.0] + [0.0] * 19, "row_den": [1.0] + [0.0] * 19}
    e, n = forward(lat + drow * MAG_PIXEL_DEG, lon + dcol * MAG_PIXEL_DEG, zone, south)
    hy = 0.015
    hx = hy * math.cos(math.radians(lat))
    return {"dsm": np.zeros((2, 2), dtype=np.float32), "bounds": [e - hx, n - hy, e + hx, n + hy], "rpc": rpc, "out_h": MAG_SIZE,
            "out_w": MAG_SIZE, "zone": zone, "south": south}


def magnifier_exact_pixels(case, easts, norths):
    """fp64 (cols, rows) of the UTM points under the case's RPC, through the exact inverse; the RPC's own arithmetic in DIGITS digits
    on the exact binary values of its fp64 entries."""
    rpc = case["rpc"]
    cols, rows = [], []
    for e, n in zip(easts, norths):
        lon, lat = inverse_mp(e, n, case["zone"], case["south"])
        with mp.workdps(DIGITS):
            cols.append(float((lon - mp.mpf(rpc["lon_offset"])) / mp.mpf(rpc["lon_scale"]) * mp.mpf(rpc["col_scale"]) + mp.mpf(rpc["col_offset"])))
            rows.append(float((lat - mp.mpf(rpc["lat_offset"])) / mp.mpf(rpc["lat_scale"]) * mp.mpf(rpc["row_scale"]) + mp.mpf(rpc["row_offset"])))
    return cols, rows


# ----------------------------------------------------------------------------- scenes that straddle a zone boundary or the equator
ZONE_SCENE_SIZE = 640          # px: a 0.3 m frame of ~190 m, +-0.001 degrees about its centre


def zone_scene(kind):
    """rpcm-format RPCs (oracle.raygen_oracle.synthetic_rpc) whose pixel (0, 0) and centre fall on different sides of a boundary:
    "zone":     centred at 77.9995 W (zone 18), pixel (0, 0) at ~78.0005 W (zone 17);
    "equator":  centred at 0.0005 N, rows counted northwards, pixel (0, 0) at ~0.0004 S;
    "conflict": pixel (0, 0) in zone 18 at max_alt = 90 and in zone 17 at min_alt = -20, through a lon x alt cross term in col_num."""
    from oracle import raygen_oracle as RO
    if kind == "zone":
        return RO.synthetic_rpc(seed=21, lat0=30.33, lon0=-77.9995, size=ZONE_SCENE_SIZE)
    if kind == "equator":
        rpc = RO.synthetic_rpc(seed=22, lat0=0.0005, lon0=-81.66, size=ZONE_SCENE_SIZE)
        rpc["row_num"] = [-v for v in rpc["row_num"]]
        return rpc
    if kind == "conflict":
        rpc = RO.synthetic_rpc(seed=23, lat0=30.33, lon0=-78.0, size=ZONE_SCENE_SIZE)
        rpc["lon_offset"] = -78.0 + 0.95 * rpc["lon_scale"]
        rpc["col_num"][5] = 0.3                                                  # apply_poly: [5] x lon x alt
        return rpc
    raise KeyError(kind)
