"""GPU: mesh smoothing through the Python layer (eonerf_code_amd/mesh.py smooth_mesh, extract_mesh(smooth=...)).  The rule is pinned at
the C ABI (tests/test_smooth_gpu.py); here: that smooth_mesh is the restatement's mesh under every way of naming the grid and the
steps, what it carries over from a dict, its errors, that iterations=0 and extract_mesh(smooth=0) keep today's bits and keys, that
extract_mesh(smooth=3, components=True, simplify=2) runs the three in order, and a noisy sheet whose error ten iterations halve."""
import numpy as np
import pytest
import torch

import mesh_restated as mr
import simplify_restated as sr
import smooth_cases as sc
import smooth_restated as sm
import test_march_python_gpu as tmp_

pytestmark = pytest.mark.gpu
N = 17
BOUNDS = ((-1.0, -0.9, -0.8), (1.0, 0.7, 0.9))
OFFSET, SCALE = (436000.25, 3355000.5, 20.0), (300.0, 250.0, 60.0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _np(t):
    return t.cpu().numpy()


def _equals(got, want, steps):
    assert _np(got["vertices"]).tobytes() == want["vertices"].tobytes()
    r = got["report"]
    assert [r[k] for k in sm.COUNTS] == want["counts"].tolist() and r["clamped"] == bool(want["status"]) and r["steps"] == list(steps)


def test_smooth_mesh_on_a_sphere_is_the_restatement_however_the_grid_and_the_steps_are_named():
    from eonerf_code_amd.mesh import MeshDict, mesh_from_volume, smooth_mesh
    origin, spacing = (-1.0, -1.0, -1.0), (0.125, 0.125, 0.125)
    v, t = mesh_from_volume(torch.from_numpy(mr.sphere_volume(N)[0]).cuda(), 0.0, origin, spacing)
    v = v + torch.from_numpy(np.random.default_rng(4).normal(0, 0.15 * 0.125, tuple(v.shape)).astype(np.float32)).cuda()
    vn, tn = _np(v), _np(t)
    got = smooth_mesh((v, t), iterations=4, origin=origin, unit=0.125)
    _equals(got, sm.smooth(vn, tn, origin, spacing, sm.taubin(4)), sm.taubin(4))
    assert set(got) == {"vertices", "faces", "report"} and got["faces"].data_ptr() == t.data_ptr() and got["report"]["free"] == v.shape[0]
    assert got["report"]["iterations"] == 4 and got["report"]["origin"] == origin and got["report"]["unit"] == spacing
    # other factors, plain Laplacian by None and by 0, three units
    _equals(smooth_mesh((v, t), iterations=3, lam=0.33, mu=-0.34, origin=origin, unit=spacing), sm.smooth(vn, tn, origin, spacing, sm.taubin(3, 0.33, -0.34)), sm.taubin(3, 0.33, -0.34))
    for mu in (None, 0, 0.0):
        _equals(smooth_mesh((v, t), iterations=5, mu=mu, origin=origin, unit=(0.125, 0.25, 0.0625)), sm.smooth(vn, tn, origin, (0.125, 0.25, 0.0625), sm.taubin(5, mu=None)),
                sm.taubin(5, mu=None))
    # a dict that knows its lattice; every other key is carried over, vertices_utm is computed again
    mesh = MeshDict({"vertices": v, "faces": t, "level": 0.0, "albedo": v * 0.5, "component": torch.arange(v.shape[0], dtype=torch.int32, device="cuda")})
    mesh.lattice = {"origin": origin, "spacing": spacing, "shape": (N, N, N)}
    mesh.scene = (torch.tensor(SCALE, dtype=torch.float64, device="cuda"), torch.tensor(OFFSET, dtype=torch.float64, device="cuda"))
    mesh["vertices_utm"] = v.double() * mesh.scene[0] + mesh.scene[1]
    by_lattice = smooth_mesh(mesh, iterations=4)
    assert torch.equal(_bits(by_lattice["vertices"]), _bits(got["vertices"]))
    assert set(by_lattice) == set(mesh) | {"report"} and by_lattice["albedo"] is mesh["albedo"] and by_lattice["component"] is mesh["component"] and by_lattice["faces"] is mesh["faces"]
    assert by_lattice.lattice == mesh.lattice and by_lattice.scene is mesh.scene and by_lattice["level"] == 0.0
    assert torch.equal(by_lattice["vertices_utm"], by_lattice["vertices"].double() * mesh.scene[0] + mesh.scene[1])
    assert torch.equal(_bits(mesh["vertices"]), _bits(v))                      # the input dict is left alone
    # the grid from the bounding box: origin at its lower corner, unit = the largest extent / 4096
    lo, hi = vn.min(axis=0), vn.max(axis=0)
    unit = max(float(h) - float(l) for h, l in zip(hi, lo)) / 4096.0
    auto = smooth_mesh((v, t), iterations=2)
    _equals(auto, sm.smooth(vn, tn, lo, (unit,) * 3, sm.taubin(2)), sm.taubin(2))
    # a mask, and open vertices
    mask = torch.zeros(v.shape[0], dtype=torch.bool, device="cuda")
    mask[::3] = True
    held = smooth_mesh((v, t), iterations=2, origin=origin, unit=0.125, pinned=mask)
    _equals(held, sm.smooth(vn, tn, origin, spacing, sm.taubin(2), pinned=_np(mask)), sm.taubin(2))
    assert torch.equal(_bits(held["vertices"][::3]), _bits(v[::3])) and held["report"]["pinned"] == int(mask.sum())
    half = t[: t.shape[0] // 2]
    for pin_open in (True, False):
        cut = smooth_mesh((v, half), iterations=2, origin=origin, unit=0.125, pin_open=pin_open)
        _equals(cut, sm.smooth(vn, _np(half), origin, spacing, sm.taubin(2), pin_open=pin_open), sm.taubin(2))
        assert cut["report"]["open"] > 0 and cut["report"]["pin_open"] is pin_open


def test_smooth_mesh_refuses_what_it_cannot_do_keeps_the_bits_at_zero_iterations_and_takes_an_empty_mesh():
    from eonerf_code_amd.mesh import smooth_mesh
    v = torch.rand(10, 3, device="cuda")
    t = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], dtype=torch.int32, device="cuda")
    for kw in (dict(lam=1.5), dict(lam=-1.01), dict(mu=-1.2), dict(mu=float("nan")), dict(lam=float("inf")), dict(unit=0.0), dict(unit=-1.0), dict(unit=(1.0, float("nan"), 1.0)),
               dict(unit=(1.0, 1.0)), dict(unit=float("inf")), dict(iterations=2049), dict(iterations=4097, mu=None), dict(iterations=-1), dict(pinned=torch.zeros(9, dtype=torch.bool)),
               dict(unit=1e-46)):
        with pytest.raises(ValueError):
            smooth_mesh((v, t), **kw)
    assert smooth_mesh((v, t), iterations=2048, unit=1.0, origin=(0, 0, 0))["report"]["steps"] == sm.taubin(2048)
    with pytest.raises(ValueError):
        smooth_mesh({"vertices": v, "faces": t, "vertices_utm": v.double()}, iterations=1)
    with pytest.raises(ValueError):
        smooth_mesh((v.cpu(), t.cpu()))
    same = smooth_mesh({"vertices": v, "faces": t, "vertices_utm": v.double(), "level": 1.0}, iterations=0)
    assert same["vertices"].data_ptr() == v.data_ptr() and same["faces"].data_ptr() == t.data_ptr() and set(same) == {"vertices", "faces", "vertices_utm", "level"}
    pair = smooth_mesh((v, t), iterations=0)
    assert torch.equal(_bits(pair["vertices"]), _bits(v)) and torch.equal(pair["faces"], t)
    empty = smooth_mesh((v[:0], t[:0]), iterations=3)
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and empty["report"]["free"] == 0 and not empty["report"]["clamped"]
    bad = v.clone()
    bad[4, 1] = float("nan")
    faces = torch.cat([t, torch.tensor([[3, 4, 5], [0, 1, 99]], dtype=torch.int32, device="cuda")])
    got = smooth_mesh((bad, faces), iterations=2, origin=(0, 0, 0), unit=1.0 / 64)
    _equals(got, sm.smooth(_np(bad), _np(faces), (0, 0, 0), (1.0 / 64,) * 3, sm.taubin(2)), sm.taubin(2))
    assert got["report"]["dead_faces"] == 2 and got["report"]["not_quantisable"] == 1 and got["report"]["free"] == 4 and got["report"]["no_corner"] == 5
    assert torch.equal(_bits(got["vertices"][4:]), _bits(bad[4:]))


def test_extract_mesh_with_smooth_and_its_default():
    from eonerf_code_amd.mesh import density_volume, extract_mesh, lattice_of, mesh_from_volume, unit_normals
    from eonerf_code_amd.normals import _axis_scale, density_gradient
    f = tmp_._field("fp32")
    origin, spacing = lattice_of(N, BOUNDS)
    vol = density_volume(f, N, BOUNDS)
    level = float(vol.median())
    v, t = mesh_from_volume(vol, level, origin, spacing)
    # smooth=0: the mesh of the volume, today's keys, today's bits
    base = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE, components=True, smooth=0)
    assert set(base) == {"vertices", "faces", "level", "normals", "albedo", "vertices_utm", "component", "component_points"}
    assert torch.equal(_bits(base["vertices"]), _bits(v)) and torch.equal(base["faces"], t) and v.shape[0] > 100
    plain = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS)
    assert set(plain) == {"vertices", "faces", "level", "normals", "albedo"} and torch.equal(_bits(plain["vertices"]), _bits(v)) and torch.equal(plain["faces"], t)
    assert torch.equal(_bits(plain["normals"]), _bits(unit_normals(density_gradient(f, v)[1])))
    # smooth alone: every vertex and face kept, positions the restatement's, normals and albedo the field's at the moved vertices
    steps = sm.taubin(3, 0.4, -0.42)
    want = sm.smooth(_np(v), _np(t), list(origin), list(spacing), steps)
    moved = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE, components=True, smooth=3, smooth_lambda=0.4, smooth_mu=-0.42)
    assert set(moved) == set(base) | {"smooth"}
    assert _np(moved["vertices"]).tobytes() == want["vertices"].tobytes() and torch.equal(moved["faces"], t) and moved["smooth"]["steps"] == steps
    assert [moved["smooth"][k] for k in sm.COUNTS] == want["counts"].tolist() and moved["smooth"]["free"] > 50
    assert not torch.equal(_bits(moved["vertices"]), _bits(v))
    assert torch.equal(moved["component"], base["component"]) and torch.equal(moved["component_points"], base["component_points"])
    assert torch.equal(_bits(moved["normals"]), _bits(unit_normals(density_gradient(f, moved["vertices"])[1], list(_axis_scale(SCALE)))))
    utm = moved["vertices"].double() * torch.tensor(SCALE, dtype=torch.float64, device="cuda") + torch.tensor(OFFSET, dtype=torch.float64, device="cuda")
    assert torch.equal(moved["vertices_utm"], utm)
    # smooth, then simplify: the restatement of the one into the restatement of the other, components through "source"
    mesh = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE, components=True, smooth=3, smooth_lambda=0.4, smooth_mu=-0.42,
                        simplify=2)
    assert set(mesh) == set(base) | {"smooth", "source", "simplify"}
    small = sr.simplify(want["vertices"], _np(t), *sr.lattice_grid(list(origin), list(spacing), (N, N, N), 2), sr.MEAN)
    assert _np(mesh["vertices"]).tobytes() == small["vertices"].tobytes() and _np(mesh["faces"]).tobytes() == small["triangles"].tobytes()
    n_out = mesh["vertices"].shape[0]
    assert 20 < n_out < v.shape[0] and mesh["simplify"]["vertices_in"] == v.shape[0] and mesh["smooth"]["vertices"] == v.shape[0]
    assert int(mesh["faces"].min()) >= 0 and int(mesh["faces"].max()) < n_out
    assert torch.equal(mesh["component"], base["component"][mesh["source"]])
    assert mesh["normals"].shape == (n_out, 3) and mesh["albedo"].shape == (n_out, 3) and mesh["vertices_utm"].shape == (n_out, 3)
    assert torch.equal(_bits(mesh["normals"]), _bits(unit_normals(density_gradient(f, mesh["vertices"])[1], list(_axis_scale(SCALE)))))


def test_ten_iterations_halve_the_error_of_a_noisy_sheet():
    """A 128 x 128 height-field sheet at z = 5 with Gaussian noise of sigma = 0.2 units on z: over the free vertices (the rim is open and
    stays) the RMS error against the plane falls to less than half.  The restatement gives 0.38 x on these very numbers, and the device
    must give the restatement's bits."""
    from eonerf_code_amd.mesh import smooth_mesh
    rng = np.random.default_rng(6)
    v, t = sc.sheet(128, 128, 5.0 + rng.normal(0, 0.2, 128 * 128))
    want = sm.smooth(v, t, (0, 0, 0), (1, 1, 1), sm.taubin(10))
    got = smooth_mesh((torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()), iterations=10, origin=(0, 0, 0), unit=1.0)
    assert _np(got["vertices"]).tobytes() == want["vertices"].tobytes()
    free = want["free"]
    assert got["report"]["free"] == int(free.sum()) == 126 * 126 and got["report"]["open"] == 4 * 127
    before = float(np.sqrt(np.mean((v[free, 2].astype(np.float64) - 5.0) ** 2)))
    after = float(np.sqrt(np.mean((_np(got["vertices"])[free, 2].astype(np.float64) - 5.0) ** 2)))
    print(f"z error over the free vertices: {before:.4f} -> {after:.4f} ({after / before:.3f} x)")
    assert 0.19 < before < 0.21 and after <= 0.5 * before
