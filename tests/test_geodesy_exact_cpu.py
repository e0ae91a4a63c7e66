"""CPU: the two numpy restatements of the UTM projection (oracle/raygen_oracle.utm_forward, tests/prior_restated.utm_inverse) and the
zone rule against references that owe nothing to them: transverse Mercator evaluated from its definition in 40-digit arithmetic
(tests/geodesy_exact.py) and the published zone rule written out as a table.

Bounds.
Forward, 1e-7 m: an fp64 ulp at 1e7 m is 1.9e-9 m, so this allows ~50 ulp of accumulated round-off; a factor 10 under the round-trip
bound of tests/test_prior_restated_cpu.py, five orders under the fp32 quantum (3-25 cm) at which the reference stores these numbers;
the n^7 truncation term of the sixth-order series is ~1e-12 m at 3 degrees off the meridian.
Inverse, 1e-12 degrees: the same length (0.1 um).
Measured (this file prints them): forward 5.6e-9 m worst with "+south" off, 2.6e-9 m with it on, 9.3e-10 m at Norway's six degrees off
the meridian; inverse 1.4e-14 degrees either way (one ulp of the longitude)."""
import mpmath as mp
import numpy as np
import pytest

import geodesy_exact as G
import prior_restated as R
from oracle import raygen_oracle as RO

FORWARD_TOL_M = 1e-7
INVERSE_TOL_DEG = 1e-12


# ----------------------------------------------------------------------------------------------------------- 1. the helper itself
def test_exact_helper_meets_tables_and_inverts_itself():
    # Meridian arc lengths on WGS84, equator -> 30 N and -> 45 N, as geodesy tables print them: to 1e-5 m, so a table value is known to
    # half a unit of its last digit (the 45 N entry is 2.3e-6 m above the true 4 984 944.377 977 7).  The table is therefore met through
    # an evaluation that shares nothing with the helper's quadrature -- the closed form with the incomplete elliptic integral of the
    # second kind, S = a (E(phi | e^2) - e^2 sin phi cos phi / sqrt(1 - e^2 sin^2 phi)) -- which must round to the table's digits; the
    # helper must meet THAT to 1e-6 m (it does to 1e-9, the fp64 round-off of the division by k0).
    for lat, table in ((30.0, "3320113.39794"), (45.0, "4984944.37798")):
        with mp.workdps(G.DIGITS):
            c, phi = G._c(), mp.radians(lat)
            closed = c.a * (mp.ellipe(phi, c.e2) - c.e2 * mp.sin(phi) * mp.cos(phi) / mp.sqrt(1 - c.e2 * mp.sin(phi) ** 2))
            assert mp.nstr(closed, 12, strip_zeros=False) == table
            assert abs(closed - mp.mpf(table)) <= mp.mpf("5e-6")
        arc = G.forward(lat, -81.0, 17)[1] / 0.9996
        print(f"arc to {lat} N: helper {arc!r}, closed form {mp.nstr(closed, 18)}, table {table}")
        assert abs(arc - float(closed)) < 1e-6
    for lat, zone in ((0.0, 17), (30.33, 17), (-79.9, 31), (84.0, 60)):
        e, n = G.forward(lat, float(G.central_meridian(zone)), zone, lat < 0)
        assert e == 500000.0                                                   # on the central meridian, exactly
    assert G.forward(0.0, 15.0, 33) == (500000.0, 0.0) and G.forward(0.0, 15.0, 33, True) == (500000.0, 10000000.0)
    for lat, lon, zone, south in ((1e-9, -173.5, 1, False), (-79.9, -0.5, 31, True), G.NORWAY, (84.0, 177.000001, 60, False),
                                  (-0.001, 21.0, 34, True), (30.33, -81.66, 17, True)):
        with mp.workdps(G.DIGITS):
            e, n = G.forward_mp(lat, lon, zone, south)
            lon2, lat2 = G._inverse_mp(e, n, zone, south)                     # the unrounded image: fp64 rounding would hide 1e-25
            assert abs(lat2 - mp.mpf(lat)) <= mp.mpf("1e-25") * abs(mp.mpf(lat))
            assert abs(lon2 - mp.mpf(lon)) <= mp.mpf("1e-25") * abs(mp.mpf(lon))


def test_point_list_covers_what_it_claims():
    pts = G.point_list()
    assert 150 <= len(pts) <= 160 and len(set(pts)) == len(pts)
    for zone in G.ZONES:
        mine = [p for p in pts if p[2] == zone]
        assert {p[0] for p in mine} >= set(G.LATS)
        assert {round(p[1] - G.central_meridian(zone), 9) for p in mine} >= set(G.DLONS)
        assert {p[3] for p in mine} == {False, True}
    assert G.NORWAY in pts and abs(G.NORWAY[1] - G.central_meridian(32)) == 6.0
    assert any(p[0] > 0 and p[3] for p in pts) and any(p[0] < 0 and not p[3] for p in pts)     # "+south" decides, not the latitude


# ----------------------------------------------------------------------------------------------------------- 2. forward
def test_numpy_forward_series_matches_the_definition():
    worst = {False: 0.0, True: 0.0}
    norway = None
    for lat, lon, zone, south in G.point_list():
        e, n = RO.utm_forward(np.array([lat]), np.array([lon]), zone, south)
        ex_e, ex_n = G.forward(lat, lon, zone, south)
        d = max(abs(float(e[0]) - ex_e), abs(float(n[0]) - ex_n))
        worst[south] = max(worst[south], d)
        if (lat, lon, zone, south) == G.NORWAY:
            norway = d
        assert d < FORWARD_TOL_M, (lat, lon, zone, south, d)
    print(f"utm_forward vs definition: worst {worst[False]:.3e} m (north), {worst[True]:.3e} m (south), Norway 6 deg off: {norway:.3e} m")


# ----------------------------------------------------------------------------------------------------------- 3. inverse
def inverse_points():
    """60 of the list: every third of the first 156 (all zones, both hemispheres, every offset), then the five after them that the
    stride leaves out, and the three special ones."""
    pts = G.point_list()
    return pts[0:156:3] + pts[1:156:32] + pts[156:]


def test_numpy_inverse_series_matches_the_definition():
    pts = inverse_points()
    assert len(pts) == 60
    worst = {False: 0.0, True: 0.0}
    for lat, lon, zone, south in pts:
        e, n = G.forward(lat, lon, zone, south)                                  # the exact forward image, as fp64
        lo, la = R.utm_inverse(np.array([e]), np.array([n]), zone, south)
        ex_lo, ex_la = G.inverse(e, n, zone, south)
        d = max(abs(float(lo[0]) - ex_lo), abs(float(la[0]) - ex_la))
        worst[south] = max(worst[south], d)
        assert d < INVERSE_TOL_DEG, (lat, lon, zone, south, d)
    print(f"utm_inverse vs definition: worst {worst[False]:.3e} deg (north), {worst[True]:.3e} deg (south)")


# ----------------------------------------------------------------------------------------------------------- 4. the zone rule
# (latitude, longitude) -> zone number, written out from the published rule (utm.latlon_to_zone_number): six-degree zones counted from
# 180 W, 180 E wrapping to zone 1; zone 32 widened to 3 E over 56 <= lat < 64; zones 31 / 33 / 35 / 37 over 72 <= lat <= 84 with edges at
# 9, 21, 33 and 42 E.
ZONE_TABLE = [
    (30.0, -180.0, 1), (30.0, -174.0, 2), (30.0, -78.0, 18), (30.0, -78.0 - 1e-12, 17), (30.0, 179.999, 60), (30.0, 180.0, 1),
    (56.0, 3.0, 32), (63.999, 11.999, 32), (64.0, 3.0, 31), (55.999, 5.0, 31), (60.0, 2.999, 31), (60.0, 12.0, 33),
    (72.0, 0.0, 31), (72.0, 8.999, 31), (72.0, 9.0, 33), (80.0, 20.999, 33), (80.0, 21.0, 35), (84.0, 32.999, 35), (84.0, 41.999, 37),
    (84.0, 42.0, 38), (84.01, 10.0, 32), (72.0, -0.001, 30),
]
# latitude -> south?  utm.latitude_to_zone_letter(lat) < 'N': the bands C..M lie south of the equator, N starts AT it
HEMISPHERE_TABLE = [(0.0, False), (1e-12, False), (-1e-12, True), (30.33, False), (-33.9, True)]


@pytest.mark.parametrize("lat,lon,zone", ZONE_TABLE)
def test_zone_number_follows_the_published_rule(lat, lon, zone):
    from eonerf_code_amd.datasets.satellite import utm_zone_from_lonlat
    assert utm_zone_from_lonlat(lon, lat)[0] == zone
    assert RO.utm_zone_number(lat, lon) == zone
    assert RO.utm_zone_and_hemisphere(lat, lon) == (zone, False)


@pytest.mark.parametrize("lat,south", HEMISPHERE_TABLE)
def test_hemisphere_follows_the_published_rule(lat, south):
    from eonerf_code_amd.datasets.satellite import utm_zone_from_lonlat
    assert utm_zone_from_lonlat(-81.66, lat)[1] is south
    assert RO.utm_zone_and_hemisphere(lat, -81.66) == (17, south)


def test_oracle_takes_zone_and_hemisphere_from_the_first_point():
    """sat_utils.py:107-111: element 0 of the call decides, not the RPC's centre; a first pixel that changes zone between max_alt
    and min_alt is refused (zone_scene: tests/test_geodesy_gpu.py drives the device with the same scenes)."""
    for kind, want in (("zone", (17, False)), ("equator", (17, True))):
        rpc = G.zone_scene(kind)
        assert RO.utm_zone_and_hemisphere(rpc["lat_offset"], rpc["lon_offset"]) != want      # the centre says otherwise
        assert RO.zone_of_first_point(rpc, 0.0, 0.0, -20.0, 90.0) == want
        assert RO.zone_of_first_point(rpc, 639.0, 639.0, -20.0, 90.0) != want                # the far corner lies beyond the boundary
    with pytest.raises(ValueError, match="18N at max_alt but in 17N at min_alt"):
        RO.zone_of_first_point(G.zone_scene("conflict"), 0.0, 0.0, -20.0, 90.0)


def test_oracle_per_point_stopping_is_one_call_per_pixel():
    """per_point=True of the oracle's localisation (what tests/test_geodesy_gpu.py compares k_raygen with): bit for bit the rays of one
    call per pixel, and within one fp32 quantum of the batch call, which iterates every pixel as long as the slowest."""
    rpc = G.zone_scene("zone")
    cols, rows = np.meshgrid(np.arange(8.0), np.arange(6.0))
    cols, rows = cols.flatten(), rows.flatten()
    batch = RO.get_rays(cols, rows, rpc, -20.0, 90.0, 17)
    each = np.concatenate([RO.get_rays(cols[k:k + 1], rows[k:k + 1], rpc, -20.0, 90.0, 17) for k in range(48)])
    np.testing.assert_array_equal(RO.get_rays(cols, rows, rpc, -20.0, 90.0, 17, per_point=True), each)
    assert (np.abs(batch.astype(np.float64) - each) <= np.spacing(np.abs(batch))).all()


# ----------------------------------------------------------------------------------------------------------- 5. the magnifier fixtures
@pytest.mark.parametrize("name", list(G.MAGNIFIER))
def test_magnifier_fixtures_leave_no_pixel_to_rounding(name):
    """tests/test_geodesy_gpu.py reads the inverse series of k_prior_splat off these fixtures to one 1e-10-degree pixel.  Each must put
    its 16 sample points into 16 distinct pixels of the image, none within 1e-3 px of a pixel edge (the device's round-off, an ulp of
    81 degrees / 1e-10), and the numpy restatement must agree with the exact pixel positions to 0.01 px = 1e-12 degrees."""
    c = G.magnifier_case(name)
    f = R.reproject(c["dsm"], c["bounds"], c["rpc"], c["out_h"], c["out_w"], c["zone"], c["south"], full=True)
    assert f["valid"].all() and f["valid"].size == 16
    assert len(set(zip(np.floor(f["rows"]).astype(int), np.floor(f["cols"]).astype(int)))) == 16
    assert (~np.isnan(f["raster"])).sum() == 16
    frac = np.concatenate([f["cols"], f["rows"]])
    assert np.abs(frac - np.round(frac)).min() > 1e-3
    margin = min(frac.min(), c["out_w"] - frac.max())
    assert margin > 256                                                           # well inside the image
    cols, rows = G.magnifier_exact_pixels(c, f["easts"], f["norths"])
    worst = max(np.abs(np.array(cols) - f["cols"]).max(), np.abs(np.array(rows) - f["rows"]).max())
    print(f"{name}: numpy inverse vs definition {worst:.2e} px of 1e-10 deg; points {frac.min():.0f} .. {frac.max():.0f} px")
    assert worst < INVERSE_TOL_DEG / G.MAG_PIXEL_DEG
