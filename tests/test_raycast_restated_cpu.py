"""CPU: the restatement of the ray casting rule (tests/raycast_restated.py, the brute force the device has to equal) against what is
known without it: the band a chord of a sphere leaves for the hits on an inscribed mesh, watertightness through every vertex and
edge midpoint, invariance under the order and the orientation of the faces, the analytic shadow of a plate."""
import numpy as np

import raycast_cases as rcc
import raycast_restated as rc

BANDS, RADIUS = 9, 1.0
LO, HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)


def sphere():
    v, t = rcc.uv_sphere(BANDS, RADIUS)
    return v.astype(np.float32), t


def circumradius(a, b, c):
    la, lb, lc = np.linalg.norm(b - c, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(a - b, axis=1)
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return la * lb * lc / (4 * area)


def test_hits_from_outside_lie_in_the_band_the_largest_face_leaves():
    # every point of a triangle whose vertices lie on a sphere of radius r lies between sqrt(r^2 - rho^2) and r from the centre, rho the
    # triangle's circumradius: the plane cuts the sphere in the circumcircle, and the triangle lies inside that disc
    v, t = sphere()
    v64 = v.astype(np.float64)
    r = np.linalg.norm(v64, axis=1)
    rho = circumradius(v64[t[:, 0]], v64[t[:, 1]], v64[t[:, 2]]).max()
    inner, outer = np.sqrt(r.min() ** 2 - rho ** 2), r.max()
    assert 0.9 < inner < 0.99 and abs(outer - 1) < 1e-6
    rng = np.random.default_rng(1)
    o = rng.normal(0, 1, (400, 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.6, 4.0, (400, 1))).astype(np.float32)
    target = rng.uniform(-0.3, 0.3, (400, 3))
    d = ((target - o) * rng.uniform(0.3, 2.0, (400, 1))).astype(np.float32)
    got = rc.closest(v, t, LO, HI, o, d)
    assert got["counts"].tolist() == [400, 0, 400] and got["dropped"] == 0
    at = o.astype(np.float64) + got["t"][:, None] * d.astype(np.float64)
    dist = np.linalg.norm(at, axis=1)
    assert (dist >= inner - 1e-12).all() and (dist <= outer + 1e-12).all(), (dist.min(), dist.max(), inner, outer)
    w = got["bary"].astype(np.float64)
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() < 1e-6
    corners = v64[t[got["face"]]]
    assert np.abs((corners * w[:, :, None]).sum(axis=1) - at).max() < 1e-6          # bary are the weights of A, B, C in that order
    # the far side is there too: with t_min behind the first hit the second one comes, at most a diameter further
    far = rc.closest(v, t, LO, HI, o[:50], d[:50], t_min=float(got["t"][:50].max()) * (1 + 1e-9))
    assert (far["face"][far["face"] >= 0] != got["face"][:50][far["face"] >= 0]).all()
    assert rc.occluded(v, t, LO, HI, o, d)["occluded"].all() and not rc.occluded(v, t, LO, HI, o, -d)["occluded"].any()


def test_no_miss_from_inside_through_any_vertex_or_edge_midpoint():
    v, t = sphere()
    v64 = v.astype(np.float64)
    edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
    mid = 0.5 * (v64[edges[:, 0]] + v64[edges[:, 1]])
    rng = np.random.default_rng(2)
    rand = rng.normal(0, 1, (500, 3))
    for centre in ((0.0, 0.0, 0.0), (0.25, -0.125, 0.5)):                 # both representable: the directions below are exact differences
        c = np.asarray(centre)
        targets = np.concatenate([v64, mid, c + rand])
        d = (targets - c).astype(np.float32)
        o = np.broadcast_to(c.astype(np.float32), d.shape)
        got = rc.closest(v, t, LO, HI, o, d)
        assert len(edges) == 3 * len(t) // 2 and got["counts"].tolist() == [len(d), 0, len(d)], (centre, np.nonzero(got["face"] < 0)[0][:10].tolist())
        nv = len(v)
        # through a vertex the hit is AT the vertex (t = 1 up to the rounding of the shear), on a face that has it
        assert np.abs(got["t"][:nv] - 1).max() < 1e-6 and all(k in t[f] for k, f in enumerate(got["face"][:nv]))
        assert rc.occluded(v, t, LO, HI, o, d)["occluded"].all()


def test_the_order_of_the_faces_does_not_matter():
    v, t = sphere()
    rng = np.random.default_rng(3)
    o, d = rcc.random_rays(rng, 300, LO, HI)
    base = rc.closest(v, t, LO, HI, o, d)
    assert 100 < base["counts"][2] < 300
    perm = rng.permutation(len(t))
    got = rc.closest(v, t[perm], LO, HI, o, d)
    hit = base["face"] >= 0
    assert got["t"].tobytes() == base["t"].tobytes() and np.array_equal(got["face"] >= 0, hit)
    same = perm[got["face"][hit]] == base["face"][hit]                     # a tie in t: the smaller number of either order
    assert same.sum() >= 0.95 * hit.sum() and got["bary"][hit][same].tobytes() == base["bary"][hit][same].tobytes()
    skip = rng.integers(0, len(t), len(o)).astype(np.int32)
    inverse = np.argsort(perm).astype(np.int32)
    assert np.array_equal(rc.occluded(v, t, LO, HI, o, d, skip=skip)["occluded"], rc.occluded(v, t[perm], LO, HI, o, d, skip=inverse[skip])["occluded"])


def test_flipped_faces_hit_the_same_face_within_the_corner_order_rounding():
    # (A, B, C) -> (A, C, B) negates U and exchanges V and W with exactly negated values, so COVER decides the same; det and the
    # numerator of t then add the same three terms in another order: two additions each, every term of one sign in det and at most
    # max |z| det in the numerator, hence |t - t'| <= 12 * 2^-53 * max(|Az|, |Bz|, |Cz|) (five roundings of relative 2^-53 on either side)
    v, t = sphere()
    rng = np.random.default_rng(4)
    o, d = rcc.random_rays(rng, 300, LO, HI)
    base, flip = rc.closest(v, t, LO, HI, o, d), rc.closest(v, t[:, [0, 2, 1]], LO, HI, o, d)
    assert np.array_equal(base["face"], flip["face"])
    hit = base["face"] >= 0
    o64, d64, v64 = o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64), v.astype(np.float64)
    kz = np.abs(d64).argmax(axis=1)
    rows = np.arange(len(o))
    z = (v64[t[base["face"].clip(0)]][rows, :, kz] - o64[rows, kz][:, None]) / d64[rows, kz][:, None]
    bound = 12 * 2.0 ** -53 * np.abs(z).max(axis=1)
    assert (np.abs(base["t"] - flip["t"])[hit] <= bound[hit]).all()
    assert np.abs(base["bary"][hit][:, [0, 2, 1]] - flip["bary"][hit]).max() <= 2.0 ** -22
    assert np.array_equal(rc.occluded(v, t, LO, HI, o, d)["occluded"], rc.occluded(v, t[:, [0, 2, 1]], LO, HI, o, d)["occluded"])


def test_degenerate_dropped_and_rejected():
    v, t = sphere()
    flat = np.concatenate([t, [[0, 0, 5], [3, 3, 3], [-1, 0, 1], [0, 1, len(v)]]])
    o, d = np.array([[0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], dtype=np.float32), np.array([[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, np.inf, 0]], dtype=np.float32)
    got = rc.closest(v, flat, LO, HI, o, d)
    assert got["dropped"] == 2 and got["counts"].tolist() == [4, 3, 1] and got["face"].tolist()[1:] == [-1, -1, -1] and 0 <= got["face"][0] < len(t)
    assert np.isnan(got["t"][1:]).all() and np.isnan(got["bary"][1:]).all()
    small = rc.closest(v, t, (-0.5,) * 3, (1.5,) * 3, o[:1], d[:1])          # a box that cuts the sphere: faces with a vertex outside are dropped
    assert 0 < small["dropped"] < len(t)
    cells, entries = rc.cell_entries(v, t, LO, HI, (3, 5, 7))
    assert cells.shape == (7, 5, 3) and entries == cells.sum() >= len(t)


def test_a_plate_over_the_ground_casts_the_analytic_shadow():
    size, height = 2.0, 1.0
    v, t = rcc.plate_scene(size, height)
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.uniform(-3.9, 3.9, (3000, 2)), np.zeros((3000, 1))], axis=1).astype(np.float32)
    for sun in ((0.3, 0.2, 1.0), (-1.0, 0.5, 0.8), (0.0, 0.0, 1.0)):
        s = np.asarray(sun, dtype=np.float32)
        s64 = s.astype(np.float64)
        at = g[:, :2].astype(np.float64) + s64[:2] * (height / s64[2])
        margin = 1e-6 * size                                              # at least that far from the shadow's edge
        inside = (np.abs(at) < size / 2 - margin).all(axis=1)
        sure = inside | (np.abs(at) > size / 2 + margin).any(axis=1)
        own = np.where(g[:, 0] >= g[:, 1], 0, 1).astype(np.int32)         # the ground triangle the point lies on
        got = rc.occluded(v, t, (-4, -4, 0), (4, 4, 2), g, np.broadcast_to(s, g.shape), skip=own, t_min=1e-3)
        assert 50 < inside.sum() < 400 and sure.sum() >= len(g) - 2
        assert np.array_equal(got["occluded"][sure] != 0, inside[sure]), sun
        # without the skip and the bias the ground under the ray's own origin blocks it at t = 0 -- exactly 0 where z is the ray's
        # largest axis (every sheared z is Sz * 0); along another axis t is a rounding either side of 0: why a shadow ray has a bias
        if abs(s[2]) >= abs(s[:2]).max():
            assert rc.occluded(v, t, (-4, -4, 0), (4, 4, 2), g, np.broadcast_to(s, g.shape))["occluded"].all()
