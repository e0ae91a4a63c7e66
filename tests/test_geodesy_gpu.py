"""GPU: the two UTM routines on the device -- utm_forward inside k_raygen, utm_inverse inside k_prior_splat -- against transverse Mercator
evaluated from its definition in 40-digit arithmetic (tests/geodesy_exact.py), and the choice of zone and hemisphere against the
reference's rule (the first point of the call decides, sat_utils.py:107-111).

Bounds.  Forward: 1e-7 m, as on the CPU (tests/test_geodesy_exact_cpu.py derives it).  Inverse: the kernel shows only the pixel a DSM
sample point lands in, so the pixel is made 1e-10 degrees (11 um) wide and every point must land within ONE pixel of where the exact
inverse puts it -- the quantum of that observation; the device's round-off is ~1e-3 px (an ulp of 81 degrees / 1e-10), and the
fixtures keep every point > 1e-3 px from a pixel edge (CPU test).  Zone choice: the one-fp32-quantum rule of
tests/test_raygen.py::test_hip_ray_generation_matches_oracle."""
import math

import numpy as np
import pytest
import torch

import geodesy_exact as G
import prior_restated as R
from oracle import raygen_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- 1. forward
def identity_rpc(lon0):
    """col -> longitude - lon0, row -> latitude, in degrees (apply_poly: [1] multiplies the longitude, [2] the latitude)."""
    return {"row_offset": 0.0, "col_offset": 0.0, "row_scale": 1.0, "col_scale": 1.0, "lat_offset": 0.0, "lon_offset": float(lon0),
            "alt_offset": 0.0, "lat_scale": 1.0, "lon_scale": 1.0, "alt_scale": 1.0, "col_num": [0.0, 1.0] + [0.0] * 18,
            "row_num": [0.0, 0.0, 1.0] + [0.0] * 17, "col_den": [1.0] + [0.0] * 19, "row_den": [1.0] + [0.0] * 19}


@pytest.mark.parametrize("zone", G.ZONES)
def test_forward_series_in_k_raygen_matches_the_definition(zone):
    """An identity RPC steers the kernel to the zone's points of the shared list; its east / north are compared with the exact forward
    of the lon / lat the kernel itself returns, which isolates the projection from the localisation.  Every point runs under both
    "+south" settings: the flag moves the northing by the false northing and nothing else."""
    from eonerf_code_amd.datasets.satellite import generate_rays
    pts = [p for p in G.point_list() if p[2] == zone]
    lon0 = float(G.central_meridian(zone))
    cols, rows = np.array([p[1] - lon0 for p in pts]), np.array([p[0] for p in pts])
    geo = {}
    for south in (False, True):
        g = generate_rays(identity_rpc(lon0), -1.0, 1.0, cols=cols, rows=rows, zone=zone, south=south, want_geo=True).cpu().numpy()
        assert np.abs(g[:, 0] - (lon0 + cols)).max() < 1e-12 and np.abs(g[:, 1] - rows).max() < 1e-12        # steered where asked
        worst = 0.0
        for k in range(len(pts)):
            e, n = G.forward(g[k, 1], g[k, 0], zone, south)
            worst = max(worst, abs(g[k, 2] - e), abs(g[k, 3] - n))
        print(f"zone {zone} south={south}: k_raygen utm_forward vs definition, worst {worst:.3e} m over {len(pts)} points")
        assert worst < 1e-7
        geo[south] = g
    # the false northing: exactly 1e7 m -- the kernel adds it to the same product in one more fp64 rounding -- and 0 in east
    assert np.array_equal(geo[True][:, 0:2], geo[False][:, 0:2])
    assert np.array_equal(geo[True][:, 2], geo[False][:, 2])
    assert np.array_equal(geo[True][:, 3], geo[False][:, 3] + 10000000.0)


# ---------------------------------------------------------------------------------------------------------------- 2. inverse
@pytest.mark.parametrize("name", list(G.MAGNIFIER))
def test_inverse_series_in_k_prior_splat_matches_the_definition(name):
    """The magnifier: 16 sample points of a 2 x 2 DSM around P, seen through an identity RPC whose pixels are 1e-10 degrees wide.  The
    non-NaN pixels of the raster are the sample points: all 16, nothing else, each within one pixel of the exact inverse of its UTM
    position (numpy's own linspace values, as the kernel's linspace_at restates them)."""
    from eonerf_code_amd import priors
    c = G.magnifier_case(name)
    dsm = torch.from_numpy(c["dsm"]).to(DEV)
    got = priors.reproject_dsm(dsm, c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"])
    assert got.shape == (G.MAG_SIZE, G.MAG_SIZE)
    hit = torch.nonzero(~torch.isnan(got)).cpu().numpy()                          # [k, 2] = (row, col)
    assert (got[~torch.isnan(got)] == 0.0).all()
    assert len(hit) == 16, hit
    easts, norths, _ = R.sample_points(2, 2, c["bounds"])
    cols, rows = G.magnifier_exact_pixels(c, easts, norths)
    used, exact = set(), 0
    for col, row in zip(cols, rows):
        near = [k for k in range(16) if abs(hit[k, 0] - math.floor(row)) <= 1 and abs(hit[k, 1] - math.floor(col)) <= 1]
        assert len(near) == 1, (name, col, row, hit.tolist())
        used.add(near[0])
        exact += int(hit[near[0], 0] == math.floor(row) and hit[near[0], 1] == math.floor(col))
    assert len(used) == 16                                                        # no point left out, none counted twice
    print(f"{name}: 16 / 16 sample points within one 1e-10-degree pixel of the definition, {exact} in the very pixel")


# ---------------------------------------------------------------------------------------------------------------- 3. zone choice
H, W, LO, HI = 24, 32, -20.0, 90.0          # 768 pixels: six blocks of k_raygen


def grid(h, w):
    cols, rows = np.meshgrid(np.arange(w), np.arange(h))
    return cols.flatten(), rows.flatten()


def oracle_rays(cols, rows, rpc, zone, south):
    """RO.get_rays with per_point=True.  The oracle's localisation, like rpcm's, iterates EVERY point of a call until the slowest has
    met the stopping rule, while k_raygen stops each pixel on its own residual.  Both ends satisfy the rule (squared normalised
    residual < 1e-18), but in these 640 px scenes they sit up to 1e-9 x lon_scale = 1e-7 m apart, enough to move 34 % of one direction
    component by a quantum (measured on the device and reproduced on the CPU) -- the localisation's slack, not the projection's.
    per_point=True stops the oracle where the kernel stops (tests/test_geodesy_exact_cpu.py: bit for bit one call per pixel), and what
    is left to compare is the zone, the hemisphere and the series."""
    return RO.get_rays(cols, rows, rpc, LO, HI, zone, south, per_point=True)


def assert_one_quantum(raw, ref_raw):
    """tests/test_raygen.py::test_hip_ray_generation_matches_oracle: raw rays equal or one fp32 quantum apart, rarely."""
    quantum = np.spacing(np.abs(ref_raw).astype(np.float32))
    d_raw = np.abs(raw.astype(np.float64) - ref_raw.astype(np.float64))
    print(f"raw rays: worst {np.max(d_raw / quantum):.2f} quanta, {(d_raw > 0).mean():.2e} of the entries differ; per column {(d_raw > 0).mean(0)}")
    assert (d_raw <= 1.01 * quantum).all()
    assert (d_raw > 0).mean() < 1e-3


def test_zone_comes_from_the_first_pixel_not_the_rpc_centre():
    from eonerf_code_amd.datasets.satellite import generate_rays, get_rays, utm_zone_from_lonlat
    rpc = G.zone_scene("zone")
    assert utm_zone_from_lonlat(rpc["lon_offset"], rpc["lat_offset"]) == (18, False)             # the centre: zone 18
    assert RO.zone_of_first_point(rpc, 0.0, 0.0, LO, HI) == (17, False)                           # pixel (0, 0): zone 17
    cols, rows = grid(H, W)
    ref_raw = oracle_rays(cols, rows, rpc, 17, False)
    raw = generate_rays(rpc, LO, HI, h=H, w=W).cpu().numpy()
    assert_one_quantum(raw, ref_raw)
    raw18 = generate_rays(rpc, LO, HI, h=H, w=W, zone=18, south=False).cpu().numpy()              # an explicit zone still overrides
    assert_one_quantum(raw18, oracle_rays(cols, rows, rpc, 18, False))
    assert (np.abs(raw[:, 0].astype(np.float64) - raw18[:, 0]) > 100e3).all()
    # explicit pixel lists: element 0 decides
    assert np.array_equal(get_rays(cols, rows, rpc, LO, HI).cpu().numpy(), raw)
    far = float(G.ZONE_SCENE_SIZE - 1)
    assert RO.zone_of_first_point(rpc, far, far, LO, HI) == (18, False)
    swapped = get_rays(np.concatenate([[far], cols]), np.concatenate([[far], rows]), rpc, LO, HI).cpu().numpy()
    assert np.array_equal(swapped[1:], raw18)


def test_hemisphere_comes_from_the_first_pixel_not_the_rpc_centre():
    from eonerf_code_amd.datasets.satellite import generate_rays, utm_zone_from_lonlat
    rpc = G.zone_scene("equator")
    assert utm_zone_from_lonlat(rpc["lon_offset"], rpc["lat_offset"]) == (17, False)             # the centre: north
    assert RO.zone_of_first_point(rpc, 0.0, 0.0, LO, HI) == (17, True)                            # pixel (0, 0): south
    cols, rows = grid(H, W)
    raw = generate_rays(rpc, LO, HI, h=H, w=W).cpu().numpy()
    assert_one_quantum(raw, oracle_rays(cols, rows, rpc, 17, True))
    assert (np.abs(raw[:, 1].astype(np.float64) - 1e7) < 200.0).all()                             # northings beside the false northing
    north = generate_rays(rpc, LO, HI, h=H, w=W, zone=17, south=False).cpu().numpy()
    assert (np.abs(north[:, 1]) < 200.0).all()


def test_first_pixel_changing_zone_between_the_altitudes_is_refused():
    from eonerf_code_amd.datasets.satellite import generate_rays, get_rays
    rpc = G.zone_scene("conflict")
    with pytest.raises(ValueError, match=r"zone 18N at max_alt .* zone 17N at min_alt"):
        generate_rays(rpc, LO, HI, h=H, w=W)
    with pytest.raises(ValueError, match=r"zone 18N at max_alt .* zone 17N at min_alt"):
        get_rays(np.array([0.0, 5.0]), np.array([0.0, 7.0]), rpc, LO, HI)
    with pytest.raises(ValueError, match="max_alt"):
        RO.zone_of_first_point(rpc, 0.0, 0.0, LO, HI)
    cols, rows = grid(H, W)
    raw = generate_rays(rpc, LO, HI, h=H, w=W, zone=18, south=False).cpu().numpy()               # an explicit zone is not questioned
    assert_one_quantum(raw, oracle_rays(cols, rows, rpc, 18, False))


def test_load_rays_uses_the_first_pixel_rule(tmp_path):
    import json
    from eonerf_code_amd.datasets import satellite as ds
    rpc = G.zone_scene("zone")
    p = tmp_path / "JAX_998_000_RGB.json"
    p.write_text(json.dumps({"img": "JAX_998_000_RGB.tif", "height": H, "width": W, "rpc": rpc, "min_alt": LO, "max_alt": HI,
                             "sun_elevation": 40.0, "sun_azimuth": 120.0}))
    ds.load_rays([str(p)], cache_dir=str(tmp_path / "cache"), device=DEV)
    cached = torch.load(tmp_path / "cache" / "JAX_998_000_RGB.data").numpy()
    cols, rows = grid(H, W)
    assert_one_quantum(cached, oracle_rays(cols, rows, rpc, 17, False))
