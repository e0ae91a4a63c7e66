"""CPU: properties of the numpy restatement of the mesh-DSM rule (tests/mesh_dsm_restated.py, include/eonerf_mesh_dsm.h).  The device and
the host program are compared with the restatement bit for bit elsewhere; here the restatement itself is held against what the rule
promises: an analytic plane to a derived bound, independence of the triangles' order and orientation, no cracks along shared edges, and
the counts of the shared cases (tests/mesh_dsm_cases.py)."""
import numpy as np

import mesh_dsm_cases as mc
import mesh_dsm_restated as md


def tessellated_plane(rng, n, a, b, c, lo, hi):
    """An n x n lattice over [lo, hi]^2 with jittered interior points, every coordinate a multiple of 1/64 (exact in fp32, and so are
    the products with the unit scale), each quad split along a random diagonal; altitude a * east + b * north + c rounded to fp32."""
    u = np.linspace(lo, hi, n)
    east, north = np.meshgrid(u, u, indexing="xy")
    step = (hi - lo) / (n - 1)
    jitter = rng.uniform(-0.4 * step, 0.4 * step, (2, n, n))
    jitter[:, 0, :] = jitter[:, -1, :] = jitter[:, :, 0] = jitter[:, :, -1] = 0.0
    east, north = np.round((east + jitter[0]) * 64) / 64, np.round((north + jitter[1]) * 64) / 64
    vertices = np.stack([east, north, a * east + b * north + c], 2).reshape(-1, 3).astype(np.float32)
    tris = []
    for r in range(n - 1):
        for q in range(n - 1):
            p00, p01, p10, p11 = r * n + q, r * n + q + 1, (r + 1) * n + q, (r + 1) * n + q + 1
            tris += [[p00, p01, p11], [p00, p11, p10]] if rng.integers(2) else [[p00, p01, p10], [p01, p11, p10]]
    return vertices, np.array(tris, dtype=np.int32)


def test_analytic_plane_within_the_derived_bound():
    """|dsm - plane| <= (|a| + |b|) * res / 8192 + 2^-16 + |z| * 2^-23 at every covered cell centre.  Derived, not measured: the snap
    moves a vertex by at most half a sub-pixel (res / 8192) per axis, and with it the plane through the snapped vertices by at most
    |a| + |b| times that at any point of the triangle; the altitude quantum is 2^-16 m, of which rounding takes half and the fp64
    interpolation far less than the other half; the fp32 output rounds by at most |z| * 2^-24, and the fp32 altitudes of the vertices
    themselves by as much again."""
    rng = np.random.default_rng(5)
    for a, b, c, res in ((0.75, -1.5, 20.0, 0.5), (-3.0, 2.0, -40.0, 0.25), (0.0, 0.0, 7.0, 1.0), (10.0, 10.0, 300.0, 0.3)):
        vertices, tris = tessellated_plane(rng, 9, a, b, c, 2.0, 14.0)
        xsize = ysize = int(np.ceil(16.0 / res))
        xoff, yoff = 0.0, 16.0
        r = md.rasterize(vertices, tris, mc.ONE, mc.ZERO, xoff, yoff, xsize, ysize, res)
        jj, ii = np.nonzero(r["face"] >= 0)
        east, north = xoff + (ii + 0.5) * res, yoff - (jj + 0.5) * res
        inside = (east >= 2.0) & (east <= 14.0) & (north >= 2.0) & (north <= 14.0)
        assert inside.all()
        want = a * east + b * north + c
        bound = (abs(a) + abs(b)) * res / 8192 + 2.0 ** -16 + np.abs(want) * 2.0 ** -23
        err = np.abs(r["dsm"][jj, ii].astype(np.float64) - want)
        assert (err <= bound).all(), (a, b, c, res, float((err / bound).max()))
        # and every centre strictly inside the square is covered
        j_all, i_all = np.meshgrid(np.arange(ysize), np.arange(xsize), indexing="ij")
        e_all, n_all = xoff + (i_all + 0.5) * res, yoff - (j_all + 0.5) * res
        must = (e_all > 2.0) & (e_all < 14.0) & (n_all > 2.0) & (n_all < 14.0)
        assert (r["face"][must] >= 0).all() and int(r["counts"][3]) >= int(must.sum()) > 100


def test_result_does_not_depend_on_the_order_of_the_triangles():
    for name in ("257 small triangles 33x17", "257 small triangles and a whole-grid one at twice in one wave 70x70", "coincident triangles 7x5"):
        c = next(k for k in mc.cases() if k["name"] == name)
        base = md.rasterize(c["vertices"], c["triangles"], c["scale"], c["offset"], *c["grid"])
        assert base["counts"][3] > 0
        rng = np.random.default_rng(17)
        for _ in range(3):
            perm = rng.permutation(len(c["triangles"]))
            other = md.rasterize(c["vertices"], c["triangles"][perm], c["scale"], c["offset"], *c["grid"])
            assert other["dsm"].tobytes() == base["dsm"].tobytes(), name
            assert other["counts"].tolist() == base["counts"].tolist(), name
            if name == "257 small triangles 33x17":          # no two of these triangles tie anywhere: the winner is the same triangle
                full = base["face"] >= 0
                assert np.array_equal(perm[other["face"][full]], base["face"][full])


def test_result_does_not_depend_on_the_orientation():
    for c in mc.cases():
        if len(c["triangles"]) == 0:
            continue
        base = md.rasterize(c["vertices"], c["triangles"], c["scale"], c["offset"], *c["grid"])
        flip = md.rasterize(c["vertices"], c["triangles"][:, ::-1], c["scale"], c["offset"], *c["grid"])
        assert flip["keys"].tobytes() == base["keys"].tobytes(), c["name"]
        assert flip["counts"].tolist() == base["counts"].tolist(), c["name"]


def test_fan_over_a_square_leaves_no_crack():
    """A closed square as a fan around an interior point that is itself a cell centre, with spokes that run exactly through cell centres
    (the diagonals, the horizontal and the vertical): every centre inside or on the square is covered, none outside is."""
    xs = ys = 12
    rim = [(2.5, 2.5), (6.5, 2.5), (9.5, 2.5), (9.5, 6.5), (9.5, 9.5), (6.5, 9.5), (2.5, 9.5), (2.5, 6.5)]
    pts = [(6.5, 6.5, 3.0)] + [(u, v, 1.0 + 0.25 * k) for k, (u, v) in enumerate(rim)]
    vertices = mc.uv(ys, pts)
    tris = np.array([[0, 1 + k, 1 + (k + 1) % len(rim)] for k in range(len(rim))], dtype=np.int32)
    for t in (tris, tris[:, ::-1], tris[::-1]):
        r = md.rasterize(vertices, t, mc.ONE, mc.SHIFT, *mc.grid(xs, ys))
        want = np.zeros((ys, xs), dtype=bool)
        want[2:10, 2:10] = True
        assert np.array_equal(r["face"] >= 0, want)
        assert r["counts"].tolist() == [8, 0, 0, 64]
        assert r["dsm"][6, 6] == 3.0
    # hits per cell: the spokes' cells are covered by two triangles, the hub by all eight, nothing by none
    hits = np.zeros((ys, xs), dtype=int)
    for k in range(len(tris)):
        hits += md.rasterize(vertices, tris[k:k + 1], mc.ONE, mc.SHIFT, *mc.grid(xs, ys))["face"] >= 0
    assert hits[6, 6] == 8 and (hits[2:10, 2:10] >= 1).all() and hits[3, 3] == 2 and hits[6, 3] == 2 and hits[4, 3] == 1 and hits.sum() > 64


def by_name(name):
    c = next(k for k in mc.cases() if k["name"] == name)
    return c, md.rasterize(c["vertices"], c["triangles"], c["scale"], c["offset"], *c["grid"])


def test_counts_and_winners_of_the_shared_cases():
    names = [c["name"] for c in mc.cases()]
    assert len(set(names)) == len(names)
    _, r = by_name("wholly outside on each side 8x6")
    assert r["counts"].tolist() == [4, 0, 0, 0] and np.isnan(r["dsm"]).all() and (r["face"] == -1).all()
    _, r = by_name("straddling each side and corner 8x6")
    assert r["counts"][0] == 8 and set(np.unique(r["face"])) == {-1, 0, 1, 2, 3, 4, 5, 6, 7}
    _, r = by_name("contains the whole grid 8x6")
    assert r["counts"].tolist() == [1, 0, 0, 48]
    _, r = by_name("three stacked layers 7x5")
    assert set(np.unique(r["face"])) == {-1, 1} and r["counts"][0] == 3
    _, r = by_name("coincident triangles 7x5")            # rolled: the three coincident ones are triangles 0, 1 and 3, the low one is 2
    assert set(np.unique(r["face"])) == {-1, 0}
    _, r = by_name("negative altitudes 7x5")
    assert set(np.unique(r["face"])) == {-1, 1} and np.nanmax(r["dsm"]) < 0
    _, r = by_name("altitudes at the bound 7x5")
    assert r["counts"][:3].tolist() == [2, 4, 0] and np.nanmax(r["dsm"]) == np.float32(32767.9) and np.nanmin(r["dsm"]) == np.float32(-32767.9)
    _, r = by_name("a vertical and a zero-size triangle between neighbours 7x5")
    assert r["counts"][:3].tolist() == [3, 0, 3] and r["counts"][3] == 30
    _, r = by_name("indices outside the mesh 7x5")
    assert r["counts"][:3].tolist() == [2, 4, 0] and r["counts"][3] == 30
    _, r = by_name("vertices that are not finite or beyond the fixed-point range 7x5")
    assert r["counts"][:3].tolist() == [2, 8, 0] and r["counts"][3] == 30
    _, r = by_name("coordinates exactly on the fixed-point bound 7x5")
    assert r["counts"][:3].tolist() == [1, 0, 0] and r["counts"][3] > 0
    _, r = by_name("negative northings 33x17")
    assert r["counts"][0] == 40 and r["counts"][3] > 0
    _, r = by_name("utm offsets and res 0.5 50x40")
    assert r["counts"][0] == 90 and r["counts"][3] > 0
    _, r = by_name("no triangles 5x3")
    assert r["counts"].tolist() == [0, 0, 0, 0] and np.isnan(r["dsm"]).all()
    for n in (63, 64, 65, 257):
        _, small = by_name(f"{n} small triangles 33x17")
        assert small["counts"][0] == n and small["counts"][3] > 30
        for where, extra in (("lane 0", 1), ("lane 63", 1), ("twice in one wave", 2)):
            _, r = by_name(f"{n} small triangles and a whole-grid one at {where} 70x70")
            assert r["counts"].tolist() == [n + extra, 0, 0, 4900]
    for xs, ys in ((1, 1), (3, 3), (5, 3)):
        _, a = by_name(f"one triangle {xs}x{ys} ccw")
        _, b = by_name(f"one triangle {xs}x{ys} cw")
        assert a["keys"].tobytes() == b["keys"].tobytes() and a["counts"][3] >= 1
    _, r = by_name("centre on an edge 1x1 ccw")
    assert r["counts"][3] == 1 and r["dsm"][0, 0] == 3.0          # halfway along the hypotenuse between altitudes 2 and 4
    _, r = by_name("centres on vertices and on an edge 3x3 cw")
    assert r["dsm"][0, 0] == 1.0 and r["dsm"][0, 2] == 2.0 and r["dsm"][2, 0] == 4.0 and r["dsm"][1, 1] == 3.0 and np.isnan(r["dsm"][2, 2]) and r["counts"][3] == 6
    _, r = by_name("centres on vertices and on an edge 5x3 ccw")
    assert r["dsm"][0, 4] == 2.0 and r["dsm"][2, 0] == 4.0 and r["dsm"][1, 2] == 3.0 and np.isnan(r["dsm"][1, 3]) and np.isnan(r["dsm"][2, 1])


def test_attributes_restate_the_altitude_and_refuse_bad_faces():
    c, r = by_name("straddling each side and corner 8x6")
    xoff, yoff, xsize, ysize, res = c["grid"]
    # the altitude as an attribute (here scale = 1 and no offset in z, so the fp32 z is the altitude): the same interpolation, rounded to fp32
    # without the 2^-16 quantum in between
    attr = np.stack([c["vertices"][:, 2], 2.0 * c["vertices"][:, 0] - c["vertices"][:, 1]], 1)
    out = md.attributes(c["vertices"], c["triangles"], c["scale"], c["offset"], xoff, yoff, xsize, ysize, res, r["face"], attr)
    full = r["face"] >= 0
    assert np.isnan(out[~full]).all() and np.isfinite(out[full]).all()
    assert np.abs(out[..., 0][full].astype(np.float64) - r["dsm"][full]).max() <= 2.0 ** -17 + 16 * 2.0 ** -24
    jj, ii = np.nonzero(full)
    east, north = xoff + (ii + 0.5) * res, yoff - (jj + 0.5) * res - c["offset"][1]          # the vertices' own northing
    assert np.abs(out[..., 1][full] - (2.0 * east - north)).max() <= 3 * res / 8192 + 32 * 2.0 ** -23
    face = r["face"].copy()
    face[0, 0], face[0, 1] = len(c["triangles"]), -7
    out2 = md.attributes(c["vertices"], c["triangles"], c["scale"], c["offset"], xoff, yoff, xsize, ysize, res, face, attr)
    assert np.isnan(out2[0, 0]).all() and np.isnan(out2[0, 1]).all()
