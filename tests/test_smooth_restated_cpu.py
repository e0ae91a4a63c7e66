"""CPU: the numpy restatement of the smoothing rule (tests/smooth_restated.py) held to what smoothing must be, so that "the device
equals the restatement" means something.  Every threshold was measured on a prototype of the rule before the kernels existed and is
met by the rule alone: ten lambda|mu iterations (0.5, -0.53) take a sphere perturbed by sigma = 0.15 spacings to 0.39 (33^3) and 0.43
(17^3) of its RMS radial error at a volume ratio of 1.001 and 1.006, ten plain Laplacian steps shrink the clean 17^3 sphere to 0.932."""
import numpy as np

import mesh_restated as mr
import smooth_cases as sc
import smooth_restated as sm

O, U = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def radial_rms(vertices, n):
    radius = 0.37 * (n - 1)
    centre = (n - 1) / 2 + np.array([0.137, 0.187, -0.073])
    return float(np.sqrt(np.mean((np.linalg.norm(vertices.astype(np.float64) - centre, axis=1) - radius) ** 2)))


def noisy_sphere(n, seed):
    v, t = sc.sphere(n)
    rng = np.random.default_rng(seed)
    return (v.astype(np.float64) + rng.normal(0.0, 0.15, v.shape)).astype(np.float32), t, v


def check_sphere(n, error_ratio, volume_band):
    v, t, clean = noisy_sphere(n, 5)
    got = sm.smooth(v, t, O, U, sm.taubin(10))
    assert got["status"] == 0 and got["counts"].tolist() == [len(v), 0, 0, 0, 0, 0]
    before, after = radial_rms(v, n), radial_rms(got["vertices"], n)
    ratio = mr.signed_volume(got["vertices"], t) / mr.signed_volume(clean, t)
    print(f"sphere {n}^3: RMS radial error {before:.4f} -> {after:.4f} ({after / before:.3f} x), volume ratio {ratio:.4f}")
    assert 0.14 < before < 0.16
    assert after <= error_ratio * before
    assert abs(ratio - 1.0) <= volume_band


def test_noisy_33_sphere_loses_half_its_error_and_keeps_its_volume():
    check_sphere(33, 0.5, 0.01)


def test_noisy_17_sphere():
    check_sphere(17, 0.6, 0.02)


def test_plain_laplacian_shrinks():
    v, t = sc.sphere(17)
    got = sm.smooth(v, t, O, U, sm.taubin(10, mu=None))
    ratio = mr.signed_volume(got["vertices"], t) / mr.signed_volume(v, t)
    print(f"ten Laplacian steps: volume ratio {ratio:.4f}")
    assert ratio < 0.95
    kept = sm.smooth(v, t, O, U, sm.taubin(10))
    assert abs(mr.signed_volume(kept["vertices"], t) / mr.signed_volume(v, t) - 1.0) < 0.02


def test_a_horizontal_plane_stays_on_one_z():
    rng = np.random.default_rng(3)
    v, t = sc.sheet(23, 19)
    v[:, 2] = np.float32(3.3)
    v[:, :2] += rng.normal(0, 0.2, (len(v), 2)).astype(np.float32)
    for pin_open in (True, False):
        got = sm.smooth(v, t, O, U, sm.taubin(10), pin_open=pin_open)
        z = got["vertices"][got["free"], 2]
        assert got["free"].sum() == (21 * 17 if pin_open else len(v))
        assert len(np.unique(z)) == 1 and abs(float(z[0]) - float(np.float32(3.3))) <= 2.0 ** -17
        assert (got["vertices"][~got["free"]] == v[~got["free"]]).all()


def test_lam_zero_moves_a_free_vertex_by_half_a_quantum_at_most():
    v, t, _ = noisy_sphere(17, 9)
    got = sm.smooth(v, t, O, U, [0])
    assert got["free"].all()
    assert np.abs(got["vertices"].astype(np.float64) - v.astype(np.float64)).max() <= 2.0 ** -17 + 2.0 ** -22      # (and the fp32 rounding of the result)


def test_open_vertices_of_the_cut_sphere_are_those_of_edges_without_a_reverse():
    v, t = sc.sphere(17, cut=8)
    k = sm.classify(v, t, O, U)
    rim = np.unique(mr.edge_report(t)[1])
    assert len(rim) > 0 and (np.nonzero(k["open"])[0] == rim).all()
    assert np.allclose(v[rim, 2], 8.0)
    got = sm.smooth(sc.noisy(np.random.default_rng(1), v, 0.15), t, O, U, sm.taubin(5))
    assert not got["free"][rim].any() and got["free"].sum() == len(v) - len(rim)
    moved = sm.smooth(sc.noisy(np.random.default_rng(1), v, 0.15), t, O, U, sm.taubin(5), pin_open=False)
    assert moved["free"].all() and moved["counts"][1] == len(rim)
    same = sc.noisy(np.random.default_rng(1), v, 0.15)
    assert got["vertices"][rim].tobytes() == same[rim].tobytes()


def test_balanced_vertices_are_not_open():
    by_name = {c["name"]: c for c in sc.cases()}
    for name, n_open in (("the 300-gon bipyramid", 0), ("two tetrahedra sharing a vertex", 0), ("a triangle with its opposite twin", 0), ("a closed tetrahedron", 0),
                         ("one triangle", 3), ("two triangles sharing only a vertex", 5), ("a fan of 1100 faces around one vertex", 1100), ("duplicate faces", 4)):      # (a face given twice leaves its edges unbalanced)
        c = by_name[name]
        k = sm.classify(c["vertices"], c["triangles"], c["origin"], c["unit"])
        assert int(k["open"].sum()) == n_open, (name, int(k["open"].sum()))
    c = by_name["a fan of 1100 faces around one vertex"]
    k = sm.classify(c["vertices"], c["triangles"], c["origin"], c["unit"])
    assert k["corners"][0] == 1100 and not k["open"][0] and k["free"][0] and k["free"].sum() == 1


def test_order_independence():
    v, t, _ = noisy_sphere(17, 11)
    rng = np.random.default_rng(12)
    base = sm.smooth(v, t, O, U, sm.taubin(4))
    perm = rng.permutation(len(t))
    assert sm.smooth(v, t[perm], O, U, sm.taubin(4))["vertices"].tobytes() == base["vertices"].tobytes()
    rolled = np.stack([np.roll(row, k % 3) for k, row in enumerate(t)])
    assert sm.smooth(v, rolled, O, U, sm.taubin(4))["vertices"].tobytes() == base["vertices"].tobytes()
    # relabelled vertices: new vertex j is old vertex perm[j]
    perm = rng.permutation(len(v))
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    other = sm.smooth(v[perm], inverse[t].astype(np.int32), O, U, sm.taubin(4))
    assert other["vertices"].tobytes() == base["vertices"][perm].tobytes()


def test_a_step_with_lambda_in_0_1_stays_inside_the_neighbours_box():
    v, t, _ = noisy_sphere(17, 13)
    k = sm.classify(v, t, O, U)
    lo = np.full((len(v), 3), np.iinfo(np.int64).max)
    hi = np.full((len(v), 3), np.iinfo(np.int64).min)
    for other in (k["next"], k["prev"]):
        np.minimum.at(lo, k["centre"], k["Q"][other])
        np.maximum.at(hi, k["centre"], k["Q"][other])
    for lam in (0, 1, 21845, 32768, 65535, 65536):
        q, clamped = sm.step(k["Q"], k["free"], k["corners"], k["centre"], k["next"], k["prev"], lam)
        assert not clamped
        box_lo, box_hi = np.minimum(lo, k["Q"]) - 1, np.maximum(hi, k["Q"]) + 1         # to one quantum
        assert ((q >= box_lo) & (q <= box_hi)).all(), lam
    q, _ = sm.step(k["Q"], k["free"], k["corners"], k["centre"], k["next"], k["prev"], 65536)
    assert ((q >= lo - 1) & (q <= hi + 1)).all()                                       # lambda = 1: the neighbours' mean itself


def test_rdiv_is_floor_division_rounded_half_up():
    assert [sm.rdiv(a, 4) for a in (-7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7)] == [-2, -1, -1, -1, -1, 0, 0, 0, 0, 1, 1, 1, 2, 2]
    a = np.array([-(1 << 62) + 1, (1 << 62) - 1, -3, 3], dtype=np.int64)
    assert sm.rdiv(a, np.int64(2)).tolist() == [-(1 << 61) + 1, 1 << 61, -1, 2]
    assert sm.rdiv(np.int64(-32768), sm.ONE) == 0 and sm.rdiv(np.int64(-32769), sm.ONE) == -1 and sm.rdiv(np.int64(32768), sm.ONE) == 1


def test_the_clamp_and_the_cases_listed():
    by_name = {c["name"]: c for c in sc.cases()}
    c = by_name["a tetrahedron near +8191.9 units under lam_q = -65536: the clamp"]
    got = sm.smooth(c["vertices"], c["triangles"], c["origin"], c["unit"], c["steps"], return_q=True)
    assert got["status"] == sm.STATUS_CLAMPED and (np.abs(got["Q"]) <= sm.LIM).all() and (np.abs(got["Q"]) == sm.LIM).any()
    c = by_name["NaN and inf vertices and two at |u| = 8192"]
    got = sm.smooth(c["vertices"], c["triangles"], c["origin"], c["unit"], c["steps"])
    assert got["counts"][4] == 5 and got["counts"][5] > 5
    bad = [3, 40, 77, 120, 150]
    assert got["vertices"][bad].tobytes() == c["vertices"][bad].tobytes()
    c = by_name["indices -1, V and 2^31 - 1"]
    assert sm.smooth(c["vertices"], c["triangles"], c["origin"], c["unit"], c["steps"])["counts"][5] == 4
    big = [c for c in sc.cases() if c["big"]]
    assert len(big) == 2 and len(big[0]["triangles"]) == 351122 and 3 * len(big[0]["triangles"]) > 1024 * 1024 and len(big[1]["vertices"]) > 1024 * 1024
    assert len(by_name["a sheet of 1025 vertices"]["vertices"]) == 1025
    for c in sc.cases():
        if not c["big"]:
            # every vertex is free, held by the mask, without a corner, not quantisable, or held as open alone
            k = sm.classify(c["vertices"], c["triangles"], c["origin"], c["unit"], c["pinned"], c["pin_open"])
            masked = np.zeros(len(c["vertices"]), dtype=bool) if c["pinned"] is None else c["pinned"] != 0
            open_alone = k["open"] & ~masked & c["pin_open"]
            assert k["counts"][0] + k["counts"][2:5].sum() + open_alone.sum() == len(c["vertices"]), c["name"]
            assert not (k["free"] & open_alone).any() and k["counts"][5] == (~k["live"]).sum() and k["counts"][0] == k["free"].sum()
