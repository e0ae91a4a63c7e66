"""GPU: mesh simplification through the Python layer (eonerf_code_amd/mesh.py simplify_mesh, extract_mesh(simplify=...)).  The rule is
pinned at the C ABI (tests/test_simplify_gpu.py); here: that simplify_mesh is the restatement's mesh under every way of naming the grid,
what it does with the per-vertex tables of a dict, that extract_mesh(simplify=2) takes normals at the new vertices and components through
"source", that the default extract_mesh has not moved, a simplified tilted plane seen from above to a derived bound, and the PLY file."""
import numpy as np
import pytest
import torch

import mesh_restated as mr
import simplify_restated as sr
import test_march_python_gpu as tmp_
import test_simplify_restated_cpu as plane

pytestmark = pytest.mark.gpu
N = 17
BOUNDS = ((-1.0, -0.9, -0.8), (1.0, 0.7, 0.9))
OFFSET, SCALE = (436000.25, 3355000.5, 20.0), (300.0, 250.0, 60.0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _np(t):
    return t.cpu().numpy()


def _equals(got, want, map_too=False):
    assert _np(got["vertices"]).tobytes() == want["vertices"].tobytes() and _np(got["faces"]).tobytes() == want["triangles"].tobytes()
    assert got["source"].dtype == torch.int64 and np.array_equal(_np(got["source"]), want["source"])
    r = got["report"]
    assert [r["vertices"], r["faces"], r["dropped"], r["collapsed"]] == want["counts"].tolist()
    if map_too:
        assert got["vertex_map"].dtype == torch.int32 and np.array_equal(_np(got["vertex_map"]), want["vertex_map"])


def test_simplify_mesh_on_a_sphere_is_the_restatement_however_the_grid_is_named():
    from eonerf_code_amd.mesh import MeshDict, mesh_from_volume, simplify_mesh
    origin, spacing = (-1.0, -1.0, -1.0), (0.125, 0.125, 0.125)
    v, t = mesh_from_volume(torch.from_numpy(mr.sphere_volume(N)[0]).cuda(), 0.0, origin, spacing)
    assert (v.shape[0], t.shape[0]) == (1964, 3924)
    vn, tn = _np(v), _np(t)
    for mode, name in ((sr.MEAN, "mean"), (sr.NEAREST, "nearest")):
        for k, counts in ((2, (160, 316)), (3, None)):
            grid = sr.lattice_grid(origin, spacing, (N, N, N), k)
            want = sr.simplify(vn, tn, *grid, mode)
            assert counts is None or tuple(want["counts"][:2]) == counts
            got = simplify_mesh((v, t), cell=[float(c) for c in grid[1]], origin=origin, dims=grid[2], representative=name, return_map=True)
            _equals(got, want, map_too=True)
            assert got["report"]["vertices_in"] == 1964 and got["report"]["faces_in"] == 3924 and got["report"]["dims"] == tuple(grid[2])
            assert set(got) == {"vertices", "faces", "source", "report", "vertex_map"}
            mesh = MeshDict({"vertices": v, "faces": t, "level": 0.0, "albedo": v * 0.5, "component": torch.arange(v.shape[0], dtype=torch.int32, device="cuda")})
            mesh.lattice = {"origin": origin, "spacing": spacing, "shape": (N, N, N)}
            by_factor = simplify_mesh(mesh, factor=k, representative=name)
            _equals(by_factor, want)
            assert set(by_factor) == {"vertices", "faces", "source", "report", "level", "albedo", "component"} and by_factor["level"] == 0.0
            assert torch.equal(by_factor["albedo"], (v * 0.5)[by_factor["source"]]) and torch.equal(by_factor["component"].long(), by_factor["source"])
            assert by_factor.lattice == mesh.lattice
    # the grid from the bounding box: origin at its lower corner, dims what covers it
    lo, hi = vn.min(axis=0), vn.max(axis=0)
    cell = float(np.float32(0.3))
    dims = [int(np.floor((float(h) - float(l)) / cell)) + 1 for l, h in zip(lo, hi)]
    _equals(simplify_mesh((v, t), cell=0.3), sr.simplify(vn, tn, lo, (0.3, 0.3, 0.3), dims, sr.MEAN))
    # simplifying a nearest result again on the same grid changes nothing
    grid = sr.lattice_grid(origin, spacing, (N, N, N), 2)
    kw = dict(cell=[float(c) for c in grid[1]], origin=origin, dims=grid[2], representative="nearest")
    once = simplify_mesh((v, t), **kw)
    twice = simplify_mesh(once, **kw)
    assert torch.equal(_bits(twice["vertices"]), _bits(once["vertices"])) and torch.equal(twice["faces"], once["faces"])
    assert twice["report"]["collapsed"] == 0 and torch.equal(twice["source"], torch.arange(once["vertices"].shape[0], device="cuda"))


def test_simplify_mesh_refuses_what_it_cannot_do_and_takes_an_empty_mesh():
    from eonerf_code_amd.mesh import simplify_mesh
    v = torch.rand(10, 3, device="cuda")
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
    for kw in (dict(), dict(cell=0.5, factor=2), dict(factor=2), dict(cell=0.0), dict(cell=(0.5, -1.0, 0.5)), dict(cell=0.5, representative="median"),
               dict(cell=0.5, origin=(0, 0, 0), dims=(4097, 1, 1)), dict(cell=1e-6, origin=(0, 0, 0), dims=(1024, 1024, 1024))):
        with pytest.raises(ValueError):
            simplify_mesh((v, t), **kw)
    with pytest.raises(ValueError):
        simplify_mesh({"vertices": v, "faces": t, "vertices_utm": v.double()}, cell=0.5)
    kept = simplify_mesh({"vertices": v, "faces": t, "vertices_utm": v.double()}, cell=0.5, representative="nearest")
    assert torch.equal(kept["vertices_utm"], v.double()[kept["source"]])
    empty = simplify_mesh((v[:0], t[:0]), cell=0.5, return_map=True)
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and empty["source"].shape == (0,) and empty["vertex_map"].shape == (0,)
    assert empty["report"]["vertices"] == 0 and empty["report"]["faces"] == 0
    bad = v.clone()
    bad[4, 1] = float("nan")
    dropped = simplify_mesh((bad, torch.tensor([[3, 4, 5], [0, 1, 99]], dtype=torch.int32, device="cuda")), cell=10.0, origin=(0, 0, 0), dims=(1, 1, 1), return_map=True)
    assert dropped["report"]["dropped"] == 2 and dropped["vertex_map"].tolist() == [0, 0, 0, 0, -1, 0, 0, 0, 0, 0] and dropped["vertices"].shape == (1, 3)


def test_extract_mesh_with_simplify_and_its_default():
    from eonerf_code_amd.mesh import density_volume, extract_mesh, lattice_of, mesh_from_volume, unit_normals
    from eonerf_code_amd.normals import _axis_scale, density_gradient
    f = tmp_._field("fp32")
    origin, spacing = lattice_of(N, BOUNDS)
    vol = density_volume(f, N, BOUNDS)
    level = float(vol.median())
    v, t = mesh_from_volume(vol, level, origin, spacing)
    # the default: the mesh of the volume, today's keys, today's bits
    base = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE, components=True)
    assert set(base) == {"vertices", "faces", "level", "normals", "albedo", "vertices_utm", "component", "component_points"}
    assert torch.equal(_bits(base["vertices"]), _bits(v)) and torch.equal(base["faces"], t) and v.shape[0] > 100
    plain = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS)
    assert set(plain) == {"vertices", "faces", "level", "normals", "albedo"} and torch.equal(_bits(plain["vertices"]), _bits(v)) and torch.equal(plain["faces"], t)
    assert torch.equal(_bits(plain["normals"]), _bits(unit_normals(density_gradient(f, v)[1])))
    for name, mode in (("mean", sr.MEAN), ("nearest", sr.NEAREST)):
        mesh = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE, components=True, simplify=2, representative=name)
        assert set(mesh) == set(base) | {"source", "simplify"}
        want = sr.simplify(_np(v), _np(t), *sr.lattice_grid(list(origin), list(spacing), (N, N, N), 2), mode)
        assert _np(mesh["vertices"]).tobytes() == want["vertices"].tobytes() and _np(mesh["faces"]).tobytes() == want["triangles"].tobytes()
        n_out = mesh["vertices"].shape[0]
        assert 20 < n_out < v.shape[0] and mesh["simplify"]["vertices_in"] == v.shape[0] and mesh["simplify"]["faces_in"] == t.shape[0]
        assert int(mesh["faces"].min()) >= 0 and int(mesh["faces"].max()) < n_out
        assert torch.equal(mesh["component"], base["component"][mesh["source"]]) and torch.equal(mesh["component_points"], base["component_points"][mesh["source"]])
        # normals and albedo are the field's at the NEW vertices
        grad = density_gradient(f, mesh["vertices"])[1]
        assert torch.equal(_bits(mesh["normals"]), _bits(unit_normals(grad, list(_axis_scale(SCALE)))))
        assert mesh["normals"].shape == (n_out, 3) and mesh["albedo"].shape == (n_out, 3)
        utm = mesh["vertices"].double() * torch.tensor(SCALE, dtype=torch.float64, device="cuda") + torch.tensor(OFFSET, dtype=torch.float64, device="cuda")
        assert torch.equal(mesh["vertices_utm"], utm)
        if name == "nearest":
            assert torch.equal(_bits(mesh["vertices"]), _bits(v[mesh["source"]]))


def test_simplified_tilted_plane_seen_from_above_and_its_ply(tmp_path):
    """rasterize_mesh of the mean-simplified plane against the plane itself.  The bound, term by term: an output vertex is off the plane by
    at most d = (|a| + |b| + 1) * cell * 2^-15 + the input's own deviation + the fp32 rounding of its coordinates (derived in
    tests/test_simplify_restated_cpu.py), and so is every point of a triangle between such vertices; the rasteriser snaps a vertex by at
    most res / 8192 per axis (12 sub-pixel bits), which moves the altitude under a fixed point by at most (|a| + |b|) times that; its
    altitude quantum is 2^-16 m; the vertex altitudes in fp64 metres and the fp32 output round by at most |z| * 2^-23 together."""
    from eonerf_code_amd.mesh import MeshDict, mesh_from_volume, rasterize_mesh, save_ply, simplify_mesh
    a, b, n = plane.A, plane.B, plane.N
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    vol = torch.from_numpy((a * x + b * y + 7.3 - z).astype(np.float32)).cuda()
    origin, spacing = (plane.ORIGIN,) * 3, (plane.SPACING,) * 3
    c = plane.ORIGIN + plane.SPACING * 7.3 - a * plane.ORIGIN - b * plane.ORIGIN
    v, t = mesh_from_volume(vol, 0.0, origin, spacing)
    mesh = MeshDict({"vertices": v, "faces": t, "normals": torch.zeros_like(v)})
    mesh.lattice = {"origin": origin, "spacing": spacing, "shape": (n, n, n)}
    own = float(plane.plane_deviation(_np(v), c).max())
    offset, scale = (10.0, 10.0, 0.0), (1.0, 1.0, 1.0)          # positive northings; the products and sums are exact in fp64
    res, size = 0.05, 40
    for k in (2, 3):
        small = simplify_mesh(mesh, factor=k)
        assert small["report"]["dropped"] == 0 and small["vertices"].shape[0] < v.shape[0] / 3
        cell = float(small["report"]["cell"][0])
        d = (abs(a) + abs(b) + 1) * cell * 2.0 ** -15 + own + (abs(a) + abs(b) + 1) * 2.0 ** -24
        assert float(plane.plane_deviation(_np(small["vertices"]), c).max()) <= d
        out = rasterize_mesh(small, offset, scale, grid=(9.0, 11.0, size, size, res), return_face=True)
        dsm, face = _np(out["dsm"]).astype(np.float64), _np(out["face"])
        centre = (np.arange(size) + 0.5) * res
        east, north = np.meshgrid(9.0 + centre, 11.0 - centre, indexing="xy")
        want = a * (east - 10.0) + b * (north - 10.0) + c
        bound = d + (abs(a) + abs(b)) * res / 8192 + 2.0 ** -16 + np.abs(want) * 2.0 ** -23
        covered = face >= 0
        err = np.abs(dsm - want)[covered]
        print(f"k = {k}: {int(covered.sum())} cells compared, worst error {err.max():.3e}, bound {float(bound[covered].min()):.3e}")
        assert (err <= bound[covered]).all()
        # the footprint: the rectangle of the output vertices; at least 80 % of the cells whose centre lies in it are compared
        sv = _np(small["vertices"]).astype(np.float64)
        inside = (east >= sv[:, 0].min() + 10.0) & (east <= sv[:, 0].max() + 10.0) & (north >= sv[:, 1].min() + 10.0) & (north <= sv[:, 1].max() + 10.0)
        assert inside.sum() > 900 and (covered & inside).sum() >= 0.8 * inside.sum()
    # the PLY of a simplified dict
    path = str(tmp_path / "small.ply")
    small["albedo"] = torch.rand(small["vertices"].shape[0], 3, device="cuda")
    save_ply(path, small)
    got = mr.read_ply(path)
    assert np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1), _np(small["vertices"])) and got["x"].dtype == np.float32
    assert np.array_equal(got["faces"], _np(small["faces"])) and np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], 1), np.zeros((len(got["x"]), 3), np.float32))
    rgb = np.rint(np.clip(_np(small["albedo"]).astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([got["red"], got["green"], got["blue"]], 1), rgb)
