"""CPU: the numpy restatement of the dual-contouring rule (tests/dual_restated.py) against what the rule promises: Hermite points that
are marching tetrahedra's axis-edge vertices bit for bit, balanced edges whatever the gradients, one vertex per mixed cell, a box whose
faces, edges and corners survive (and which marching tetrahedra cut off: the case discriminates), a sphere, and the special values.
The GPU tests hold the library to this restatement bit for bit; this file holds the restatement to the geometry."""
import numpy as np
import pytest

import dual_cases as dc
import dual_restated as dr
import mesh_restated as mr


def contour(case, **kw):
    args = dict(level=case["level"], gradient=case["g"], origin=case["origin"], spacing=case["spacing"], regularisation=case["lam"])
    args.update(kw)
    return dr.contour(case["f"], **args)


def unit_face_normals(vertices, triangles):
    n = mr.face_normals(vertices, triangles)
    length = np.linalg.norm(n, axis=1)
    keep = length > 0
    return n[keep] / length[keep][:, None], length[keep] / 2, keep


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 4, 5), (6, 5, 7), (9, 17, 33)], ids=str)
def test_hermite_points_are_marching_tetrahedra_s_axis_edge_vertices(shape):
    f = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    f.reshape(-1)[::11] = 0.1                          # values on the level
    origin, spacing = (-1.0, -0.5, 0.25), (0.3, 0.37, -1.5)
    tetra = mr.extract(f, 0.1, origin, spacing)
    axis = (tetra["keys"] & 7) < 3
    got = dr.hermite(f, 0.1, origin, spacing)
    assert len(got["keys"]) > 0
    assert dc.same_bits(got["keys"], tetra["keys"][axis]) and dc.same_bits(got["points"], tetra["vertices"][axis])


@pytest.mark.parametrize("seed", range(4))
def test_every_directed_edge_is_balanced_whatever_the_gradients(seed):
    rng = np.random.default_rng(seed)
    f = dc.shell(rng.standard_normal((5, 6, 7)).astype(np.float32))
    r = dr.contour(f, 0.0, lambda points: rng.standard_normal((len(points), 3)).astype(np.float32), regularisation=0.1)
    assert len(r["triangles"]) == 2 * len(r["keys"]) > 0          # inside the shell every crossing edge has four cells around it
    e = mr.directed_edges(r["triangles"])
    big = len(r["vertices"])
    forward, counts = np.unique(e[:, 0] * big + e[:, 1], return_counts=True)
    backward, back_counts = np.unique(e[:, 1] * big + e[:, 0], return_counts=True)
    assert np.array_equal(forward, backward) and np.array_equal(counts, back_counts)         # as many twins as copies
    # topology does not read the gradients
    other = dr.contour(f, 0.0, np.zeros((len(r["keys"]), 3), dtype=np.float32))
    assert np.array_equal(other["triangles"], r["triangles"]) and np.array_equal(other["cell_keys"], r["cell_keys"])


def test_single_cell_under_all_256_sign_patterns():
    mag = np.random.default_rng(1).uniform(0.2, 1.7, (256, 8)).astype(np.float32)
    rng = np.random.default_rng(2)
    for pattern in range(256):
        sign = np.array([1.0 if (pattern >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)
        r = dr.contour((mag[pattern] * sign).reshape(2, 2, 2), 0.0, lambda p: rng.standard_normal((len(p), 3)).astype(np.float32))
        mixed = pattern not in (0, 255)
        assert len(r["vertices"]) == (1 if mixed else 0) and len(r["triangles"]) == 0, pattern
        assert (len(r["keys"]) > 0) == mixed
        if mixed:
            assert ((r["local"] >= 0) & (r["local"] <= 1)).all() and ((r["vertices"] >= 0) & (r["vertices"] <= 1)).all(), pattern


# The box's two faces on an axis lie the same delta outside lattice planes 3 and 9.  With EQUAL deltas every crossing edge runs from a
# value delta - 1 to a value delta, along the box's edges and corners too, so linear interpolation puts every Hermite point exactly on
# a face (t = 1 - delta or delta).  Unequal deltas on two axes would make f on an edge through the box's rim the minimum of two
# different ramps, and the crossing points near the rims would move off the faces: the bounds below would then test the field, not the mesher.
@pytest.mark.parametrize("delta", [0.25, 0.6])
def test_box_keeps_its_faces_edges_and_corners(delta):
    case = dc.box_case(delta)
    lam = case["lam"]
    r = contour(case)
    assert r["report"] == (0, 0, 0, 0)
    normals, area, keep = unit_face_normals(r["vertices"], r["triangles"])
    off_axis = 1.0 - np.abs(normals).max(axis=1)
    print(f"box delta {delta}: {len(r['vertices'])} vertices, {len(r['triangles'])} triangles, worst 1 - max|n_c| {off_axis.max():.3g}")
    assert off_axis.max() <= 1e-4                               # measured 1.9e-6 (delta 0.25) and 5.1e-6 (delta 0.6)
    lo, hi = dc.BOX_LO - delta, dc.BOX_HI + delta
    bound = np.sqrt(3.0) * lam * lam / (1.0 + lam * lam) + 1e-5          # per axis the factor k / (k + lam^2) with k >= 1 planes: 0.01715 at lam = 0.1
    worst = 0.0
    for corner in [(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)]:
        worst = max(worst, np.linalg.norm(r["vertices"].astype(np.float64) - np.array(corner), axis=1).min())
    print(f"box delta {delta}: worst corner distance {worst:.4g} (bound {bound:.4g})")
    assert worst <= bound                                       # measured 0.0029 (delta 0.25) and 0.0069 (delta 0.6)
    ratio = mr.signed_volume(r["vertices"], r["triangles"]) / (hi - lo) ** 3
    print(f"box delta {delta}: volume ratio {ratio:.6f}")
    assert 0.999 <= ratio <= 1.0 + 1e-6                         # measured 0.99986 (delta 0.25) and 0.99960 (delta 0.6)
    most, missing = mr.edge_report(r["triangles"])
    assert most == 1 and len(missing) == 0
    assert (len(r["vertices"]), len(r["triangles"])) == (296, 588)
    # the case discriminates: marching tetrahedra on the same volume cut the rims off
    tetra = mr.extract(case["f"], case["level"], case["origin"], case["spacing"])
    t_normals, t_area, _ = unit_face_normals(tetra["vertices"], tetra["triangles"])
    t_off = (1.0 - np.abs(t_normals).max(axis=1)) > 1e-4
    t_ratio = mr.signed_volume(tetra["vertices"], tetra["triangles"]) / (hi - lo) ** 3
    print(f"box delta {delta}: marching tetrahedra off-axis area {t_area[t_off].sum() / t_area.sum():.4f}, volume ratio {t_ratio:.6f}, {len(tetra['vertices'])} vertices")
    assert t_area[t_off].sum() / t_area.sum() > 0.05 and t_ratio < 0.997          # 5.4 % / 0.9957 (delta 0.25), 11.4 % / 0.9803 (delta 0.6)
    assert len(tetra["vertices"]) == 1094


def test_sphere_is_closed_oriented_and_near_the_sphere():
    case = dc.sphere_case()
    r = contour(case)
    most, missing = mr.edge_report(r["triangles"])
    assert most == 1 and len(missing) == 0                      # closed, every edge once in each direction: oriented and balanced
    assert mr.euler_characteristic(len(r["vertices"]), r["triangles"]) == 2
    assert (len(r["vertices"]), len(r["triangles"])) == (1262, 2520) and r["report"][1:] == (0, 0, 0)
    exact = 4.0 / 3.0 * np.pi * dc.SPHERE_R ** 3
    ratio = mr.signed_volume(r["vertices"], r["triangles"]) / exact
    radius = np.linalg.norm(r["vertices"].astype(np.float64) - np.array(dc.SPHERE_C), axis=1)
    print(f"sphere: |volume ratio - 1| {abs(ratio - 1):.4g}, max |r - R| {np.abs(radius - dc.SPHERE_R).max():.4g} spacings")
    assert ratio > 0
    assert abs(ratio - 1.0) <= 2 * 1.753e-3                     # twice what this restatement measures: 1.753e-3
    assert np.abs(radius - dc.SPHERE_R).max() <= 2 * 0.03935    # twice what this restatement measures: 0.03935 spacings
    tetra = mr.extract(case["f"], case["level"])
    assert len(r["triangles"]) < 0.4 * len(tetra["triangles"])  # 2,520 against 7,528


def test_values_equal_to_the_level():
    r = contour(dc.level_case())
    assert len(r["triangles"]) > 0 and r["nonfinite"] == 0
    star = np.full((3, 3, 3), -1.0, dtype=np.float32)
    star[1, 1, 1] = 0.0                                         # one point ON the level is inside: six Hermite points, all at the point itself
    r = dr.contour(star, 0.0, np.tile(np.array([[1.0, 0.0, 0.0]], dtype=np.float32), (6, 1)))
    assert dr.counts_of(r) == (6, 8, 12, 0) and (r["points"] == 1.0).all()
    assert (r["vertices"] == 1.0).all()                         # every q_e of every cell is the point: m is, and b = 0
    assert (np.linalg.norm(mr.face_normals(r["vertices"], r["triangles"]), axis=1) == 0).all()      # degenerate triangles are kept


def test_values_that_are_not_finite():
    case = dc.nonfinite_value_case()
    r = contour(case)
    assert r["nonfinite"] > 10 and np.isfinite(r["vertices"]).all() and np.isfinite(r["points"]).all()
    f = np.full((3, 3, 3), -1.0, dtype=np.float32)
    f[1, 1, 1] = np.inf
    r = dr.contour(f, 0.0, np.ones((6, 3), dtype=np.float32))
    assert dr.counts_of(r) == (6, 8, 12, 6)
    assert sorted(np.abs(r["points"] - 1.0).sum(axis=1).tolist()) == [0.5] * 6           # t = 0.5 on every edge
    f[1, 1, 1] = np.nan                                         # a NaN is outside
    r = dr.contour(f, 0.0, np.zeros((0, 3), dtype=np.float32))
    assert dr.counts_of(r) == (0, 0, 0, 0)


def test_gradients_that_are_zero_nan_or_infinite_are_dropped_and_counted():
    case = dc.bad_gradient_case()
    r = contour(case)
    g = case["g"]
    bad = ~np.isfinite(g).all(axis=1) | (g == 0).all(axis=1)
    assert bad.sum() >= 4 * (len(g) // 8) > 0
    # every Hermite point lies on an edge shared by up to four cells; the dropped counter counts (cell, edge) pairs
    ids = {int(k): n for n, k in enumerate(r["keys"])}
    nz, ny, nx = case["f"].shape
    uses = np.zeros(len(g), dtype=np.int64)
    for cell in r["cell_keys"]:
        for e in range(12):
            a, off = dr.edge_of(e)
            key = (int(cell) + off[0] + off[1] * nx + off[2] * nx * ny) * 8 + a
            if key in ids:
                uses[ids[key]] += 1
    assert r["report"][2] == int(uses[bad].sum()) > 0 and r["report"][1] == 0
    assert np.isfinite(r["vertices"]).all()
    good = np.where(bad[:, None], np.float32(0), g)             # a dropped plane is a zero gradient: same vertices
    assert dc.same_bits(contour(case, gradient=good)["vertices"], r["vertices"])


def test_a_cell_with_no_usable_plane_gives_the_mean_of_its_hermite_points():
    case = dc.no_plane_case()
    r = contour(case)
    assert r["report"][2] > 0 and r["report"][:2] == (0, 0)
    nz, ny, nx = case["f"].shape
    ids = {int(k): n for n, k in enumerate(r["keys"])}
    for v, cell in enumerate(r["cell_keys"]):
        i, j, k = int(cell) % nx, int(cell) // nx % ny, int(cell) // (nx * ny)
        rows = [ids[(int(cell) + off[0] + off[1] * nx + off[2] * nx * ny) * 8 + a] for a, off in map(dr.edge_of, range(12))
                if (int(cell) + off[0] + off[1] * nx + off[2] * nx * ny) * 8 + a in ids]
        mean = r["points"][rows].astype(np.float64).mean(axis=0) - np.array([i, j, k])
        assert np.abs(r["local"][v] - mean).max() < 1e-6, v    # (unit lattice: a Hermite point's cell-local coordinate is its position minus the corner)


def test_regularisation_at_both_ends_of_its_range():
    tight = contour(dc.random_case((4, 5, 6), lam=dr.MAX_REGULARISATION))
    loose = contour(dc.random_case((4, 5, 6), lam=dr.MIN_REGULARISATION))
    mean = contour(dc.random_case((4, 5, 6)), gradient=np.zeros_like(dc.random_case((4, 5, 6))["g"]))
    assert np.array_equal(tight["triangles"], loose["triangles"])
    # lambda = 16: x - m = A^-1 b with A >= 256 I and |b| <= 12 sqrt(3): within 0.09 of the mean; lambda = 2^-10 moves further
    assert np.abs(tight["local"] - mean["local"]).max() < 0.09 < np.abs(loose["local"] - mean["local"]).max()
    assert tight["report"][0] == 0 and loose["report"][0] > 0 and np.isfinite(loose["vertices"]).all()
    for lam in (dr.MIN_REGULARISATION / 2, 2 * dr.MAX_REGULARISATION, float("nan")):
        with pytest.raises(AssertionError):
            contour(dc.random_case((2, 2, 2)), regularisation=lam)


def test_capacity_semantics_of_the_counts():
    """What a capacity one too small cuts off is the LAST id: ids are dense and in key order (the GPU test checks the library's side)."""
    r = contour(dc.random_case((3, 4, 5)))
    assert np.all(np.diff(r["keys"]) > 0) and np.all(np.diff(r["cell_keys"]) > 0)
    assert r["triangles"].min() >= 0 and r["triangles"].max() < len(r["vertices"])
    assert dr.counts_of(r) == (len(r["points"]), len(r["vertices"]), len(r["triangles"]), 0)
