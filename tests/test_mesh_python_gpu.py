"""GPU: mesh export through the Python layer (eonerf_code_amd/mesh.py) on random-weight fields, 17^3 lattice points.  The rule is pinned
at the C ABI (tests/test_mesh_gpu.py); here: that the density volume is field.query_density's bit for bit whatever the slab size, that
mesh_from_volume is the restatement's mesh of that volume, that normals, albedo and UTM vertices of extract_mesh are what their
definitions say, the PLY file, and the context a bf16 field runs on."""
import numpy as np
import pytest
import torch

import mesh_restated as mr
import test_march_python_gpu as tmp_

pytestmark = pytest.mark.gpu
N = 17
BOUNDS = ((-1.0, -0.9, -0.8), (1.0, 0.7, 0.9))
OFFSET, SCALE = (436000.25, 3355000.5, 20.0), (300.0, 250.0, 60.0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _lattice(bounds=BOUNDS, n=N):
    from eonerf_code_amd.mesh import lattice_of
    origin, spacing = lattice_of(n, bounds)
    return origin, spacing, torch.from_numpy(mr.lattice_points(np.array(list(origin), dtype=np.float32), np.array(list(spacing), dtype=np.float32), n, n, 0, n)).cuda()


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_volume_mesh_normals_albedo_and_ply(precision, tmp_path):
    from eonerf_code_amd.mesh import density_volume, extract_mesh, mesh_from_volume, save_ply
    from eonerf_code_amd.normals import density_gradient
    f = tmp_._field(precision)
    assert f.training                                   # a module in training mode: the export calls must not depend on it, nor change it
    origin, spacing, xyz = _lattice()
    assert list(origin) == [np.float32(v) for v in BOUNDS[0]]
    with torch.no_grad():
        f.eval()
        want = f.query_density(xyz.reshape(-1, 3)).reshape(N, N, N)
        f.train()
    vol = density_volume(f, N, BOUNDS)
    assert vol.shape == (N, N, N) and vol.dtype == torch.float32 and torch.equal(_bits(vol), _bits(want))
    for slab_points in (1, 2 * N * N + 5, 1 << 30):      # one layer per call, two layers and a ragged rest, everything at once
        assert torch.equal(_bits(density_volume(f, (N, N, N), BOUNDS, slab_points=slab_points)), _bits(want))
    assert f.training

    level = float(vol.median())
    v, t, k = mesh_from_volume(vol, level, origin, spacing, return_keys=True)
    ref = mr.extract(vol.cpu().numpy(), level, list(origin), list(spacing))
    assert len(ref["keys"]) > 100 and len(ref["triangles"]) > 100
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.shape == (len(ref["keys"]), 3) and t.shape == (len(ref["triangles"]), 3)
    assert v.cpu().numpy().tobytes() == ref["vertices"].tobytes() and np.array_equal(k.cpu().numpy(), ref["keys"])
    assert np.array_equal(mr.rotate_smallest_first(t.cpu().numpy()), mr.rotate_smallest_first(ref["triangles"]))

    mesh = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, scene_offset=OFFSET, scene_scale=SCALE)
    assert set(mesh) == {"vertices", "faces", "level", "normals", "albedo", "vertices_utm"} and mesh["level"] == level and f.training
    assert torch.equal(_bits(mesh["vertices"]), _bits(v)) and torch.equal(mesh["faces"], t)
    # normals: -grad sigma / |grad sigma| with the gradient first taken to the metric frame (times 1 / scene_scale)
    _, grad = density_gradient(f, v)
    g = grad * torch.tensor([np.float32(1.0 / s) for s in SCALE], device="cuda")
    length = torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    ok = (length > 0) & torch.isfinite(length)
    unit = torch.where(ok[:, None], -g / length[:, None], torch.zeros_like(g))
    assert int(ok.sum()) > 100 and torch.equal(_bits(mesh["normals"]), _bits(unit))
    assert bool(((torch.linalg.vector_norm(mesh["normals"][ok], dim=1) - 1).abs() <= 12 * 2.0 ** -24).all())
    # albedo: the field's forward at the vertices, in eval mode; the sun direction and the image index do not enter that head
    with torch.no_grad():
        f.eval()
        sun = torch.tensor([0.3, -0.2, 0.93], device="cuda").expand(v.shape[0], 3)
        alb = f(v, sun, torch.full((v.shape[0],), 3, dtype=torch.int64, device="cuda"))[1]
        f.train()
    assert torch.equal(_bits(mesh["albedo"]), _bits(alb))
    utm = v.double() * torch.tensor(SCALE, dtype=torch.float64, device="cuda") + torch.tensor(OFFSET, dtype=torch.float64, device="cuda")
    assert mesh["vertices_utm"].dtype == torch.float64 and torch.equal(mesh["vertices_utm"], utm)
    bare = extract_mesh(f, resolution=N, level=level, bounds=BOUNDS, normals=False, albedo=False)
    assert set(bare) == {"vertices", "faces", "level"} and torch.equal(_bits(bare["vertices"]), _bits(v))

    path = str(tmp_path / "mesh.ply")
    save_ply(path, mesh)
    got = mr.read_ply(path)
    assert np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1), utm.cpu().numpy()) and got["x"].dtype == np.float64
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], 1), mesh["normals"].cpu().numpy())
    rgb = np.rint(np.clip(alb.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([got["red"], got["green"], got["blue"]], 1), rgb) and np.array_equal(got["faces"], t.cpu().numpy())
    save_ply(path, bare)
    got = mr.read_ply(path)
    assert got["x"].dtype == np.float32 and np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1), v.cpu().numpy()) and "nx" not in got


def test_a_bf16_field_follows_the_context_choice_of_render_normals():
    from eonerf_code_amd.mesh import density_volume, extract_mesh
    from eonerf_code_amd.normals import density_gradient
    _, _, xyz = _lattice()
    # the default: a bf16 field exports on its fp16x3 context, as its renders and its eval-mode query_density do
    bf = tmp_._field("bf16")
    vol = density_volume(bf, N, BOUNDS)
    with torch.no_grad():
        want = bf.eval().query_density(xyz.reshape(-1, 3)).reshape(N, N, N)
        bf.train()
    assert bf._ctx_eval is not None and bf.eval_precision == "fp16x3" and torch.equal(_bits(vol), _bits(want))
    assert torch.equal(_bits(vol), _bits(density_volume(tmp_._field("fp16x3"), N, BOUNDS)))
    # eval_precision "same": there is no bf16 gradient, so render_normals / density_gradient run on an fp32 context -- and so does the volume
    same = tmp_._field("bf16", eval_precision="same")
    vol = density_volume(same, N, BOUNDS)
    f32 = tmp_._field("fp32")
    assert torch.equal(_bits(vol), _bits(density_volume(f32, N, BOUNDS)))
    sigma, _ = density_gradient(same, xyz.reshape(-1, 3))
    assert torch.equal(_bits(vol.reshape(-1)), _bits(sigma.reshape(-1)))
    with torch.no_grad():
        assert same._native(True)[0] is same._ctx          # the bf16 field's own renders stay where they were
    level = float(vol.median())
    a, b = extract_mesh(same, resolution=N, level=level, bounds=BOUNDS), extract_mesh(f32, resolution=N, level=level, bounds=BOUNDS)
    assert a["vertices"].shape[0] > 100
    for name in ("vertices", "normals"):                   # (the albedo is the field's own forward: bf16 there)
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    assert torch.equal(a["faces"], b["faces"])


def test_shapes_and_arguments_are_checked():
    from eonerf_code_amd.mesh import density_volume, level_from_opacity, mesh_from_volume
    f = tmp_._field("fp32")
    vol = density_volume(f, (3, 4, 5), ((-1, -1, -1), (1, 1, 1)))
    assert vol.shape == (3, 4, 5)
    with pytest.raises(ValueError):
        density_volume(f, (1, 4, 5))
    with pytest.raises(ValueError):
        density_volume(f, 5, ((-1, -1, -1), (1, -1, 1)))
    with pytest.raises(ValueError):
        mesh_from_volume(vol.cpu(), 0.0)
    v, t = mesh_from_volume(torch.full((3, 4, 5), -1.0, device="cuda"), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    assert level_from_opacity(0.5, 2 / 128) == pytest.approx(44.3614, rel=1e-5)
