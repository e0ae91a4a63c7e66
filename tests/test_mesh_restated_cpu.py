"""CPU: the mesh rule as restated in numpy (tests/mesh_restated.py) -- spheres, a plane, a random volume -- the binding's symbol list
against the new header, and the PLY writer.  The device tests (tests/test_mesh_gpu.py) compare the library with this restatement bit
for bit; here the restatement itself is held to what a mesh must be: closed, oriented, of the right volume."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_restated as mr
from conftest import REPO

# vertices, triangles of the rule on the sphere f = R^2 - |x - c|^2 at level 0, measured once on a numpy prototype of the rule
SPHERES = {9: (472, 940), 17: (1964, 3924), 33: (7838, 15672)}


@pytest.fixture(scope="module")
def spheres():
    out = {}
    for n in SPHERES:
        f, radius = mr.sphere_volume(n)
        out[n] = (mr.extract(f, 0.0), radius)
    return out


@pytest.mark.parametrize("n", sorted(SPHERES))
def test_sphere_is_a_closed_oriented_surface_with_the_listed_counts(spheres, n):
    m, radius = spheres[n]
    v, t = m["vertices"], m["triangles"]
    assert (len(v), len(t)) == SPHERES[n] and m["nonfinite"] == 0
    most, unpaired = mr.edge_report(t)
    assert most == 1 and len(unpaired) == 0          # every undirected edge in exactly two triangles, once per direction
    assert mr.euler_characteristic(len(v), t) == 2
    assert (np.linalg.norm(mr.face_normals(v, t), axis=1) > 0).all()
    assert len(np.unique(v, axis=0)) == len(v)
    assert mr.signed_volume(v, t) > 0


def test_sphere_volume_error_is_negative_and_second_order(spheres):
    err = {}
    for n, (m, radius) in spheres.items():
        exact = 4.0 / 3.0 * np.pi * radius ** 3
        err[n] = (mr.signed_volume(m["vertices"], m["triangles"]) - exact) / exact
        print(f"{n}^3: volume error {100 * err[n]:+.3f} %")
    assert all(e < 0 for e in err.values()) and abs(err[9]) <= 0.10
    assert 3.0 <= err[9] / err[17] <= 5.0 and 3.0 <= err[17] / err[33] <= 5.0


def test_plane_off_the_lattice():
    nx, ny, nz, z0, level = 7, 6, 5, 1.7, 0.3
    z = np.arange(nz, dtype=np.float32)[:, None, None]
    f = (np.float32(level) + (np.float32(z0) - z)).astype(np.float32) * np.ones((nz, ny, nx), dtype=np.float32)
    m = mr.extract(f, level)
    v, t = m["vertices"], m["triangles"]
    # a horizontal plane cuts the six tetrahedra of a cell in 1 + 2 + 1 + 2 + 1 + 1 triangles (z last, second, last, second, first, first
    # on the path) and crosses every edge that steps in z: slots 2, 4, 5, 6
    assert len(t) == 8 * (nx - 1) * (ny - 1) and len(v) == nx * ny + (nx - 1) * ny + nx * (ny - 1) + (nx - 1) * (ny - 1)
    ulp = np.spacing(np.float32(z0))
    assert (np.abs(v[:, 2] - np.float32(z0)) <= ulp).all()
    normals = mr.face_normals(v, t)
    assert (normals[:, 2] > 0).all() and (normals[:, :2] == 0).all()        # the dense side is below: normals point up
    most, unpaired = mr.edge_report(t)
    assert most == 1 and len(unpaired) > 0
    ends = v[unpaired]                                                      # [m, 2, 3]: a boundary edge lies on one face of the volume
    on_face = [(ends[:, :, a] == b).all(axis=1) for a, b in ((0, 0), (0, nx - 1), (1, 0), (1, ny - 1))]
    assert np.logical_or.reduce(on_face).all()


def test_random_volume_has_no_directed_edge_twice():
    f = np.random.default_rng(5).standard_normal((4, 5, 6)).astype(np.float32)
    m = mr.extract(f, 0.0)
    assert len(m["triangles"]) > 100
    most, _ = mr.edge_report(m["triangles"])
    assert most == 1
    assert (np.diff(m["keys"]) > 0).all() and len(m["keys"]) == len(m["vertices"])


def test_values_on_the_level_and_values_that_are_not_finite():
    f = np.full((3, 3, 3), -1.0, dtype=np.float32)
    f[1, 1, 1] = 0.0                                 # equal to the level: inside, every vertex of its star sits on the point itself
    m = mr.extract(f, 0.0)
    assert len(m["vertices"]) == 14 and (m["vertices"] == 1.0).all() and m["nonfinite"] == 0
    assert len(m["triangles"]) == 24 and (np.linalg.norm(mr.face_normals(m["vertices"], m["triangles"]), axis=1) == 0).all()
    f[1, 1, 1] = np.inf
    m = mr.extract(f, 0.0)
    assert m["nonfinite"] == 14 and len(m["triangles"]) == 24
    assert sorted(np.abs(m["vertices"] - 1.0).max(axis=1).tolist()) == [0.5] * 14
    most, unpaired = mr.edge_report(m["triangles"])
    assert most == 1 and len(unpaired) == 0 and mr.signed_volume(m["vertices"], m["triangles"]) > 0
    f[1, 1, 1] = np.nan                              # a NaN is outside
    assert len(mr.extract(f, 0.0)["triangles"]) == 0


def test_table_has_the_rules_shape():
    assert mr.PERMS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for path, cases in zip(mr.PATHS, mr.TABLE):
        assert path[0] == (0, 0, 0) and path[3] == (1, 1, 1)
        assert [len(c) for c in cases] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def test_restatement_imports_nothing_from_the_product_path():
    src = open(os.path.join(REPO, "tests", "mesh_restated.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", src, flags=re.M) == ["itertools", "numpy"]


# ---- header pins ------------------------------------------------------------------------------------------------------------------
def test_mesh_header_symbols_are_bound_and_exported():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(REPO, "include", "eonerf_mesh.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.eonerf_mesh_version.restype = ctypes.c_int
    assert L.eonerf_mesh_version() == 1
    assert int(re.search(r"#define\s+EONERF_MESH_VERSION\s+(\d+)", hdr).group(1)) == 1
    assert re.search(r"#define\s+EONERF_MESH_MAX_POINTS\s+\(1 << 28\)", hdr)
    L.eonerf_version.restype = ctypes.c_int
    assert L.eonerf_version() == 502
    L.eonerf_mesh_workspace_bytes.restype = ctypes.c_size_t
    wb = L.eonerf_mesh_workspace_bytes
    assert wb(1, 2, 2) == 0 and wb(2, 2, 1) == 0 and wb((1 << 14) + 1, 1 << 13, 2) == 0 and wb(1 << 16, 1 << 16, 1 << 16) == 0
    assert wb(2, 2, 2) == 1536 and wb(1 << 14, 1 << 13, 2) > 5 << 28


# ---- the PLY writer ---------------------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    from eonerf_code_amd.mesh import level_from_opacity, save_ply
    m = mr.extract(mr.sphere_volume(9)[0], 0.0, origin=(-1, -1, -1), spacing=(0.25, 0.25, 0.25))
    rng = np.random.default_rng(2)
    normals = rng.standard_normal((len(m["vertices"]), 3)).astype(np.float32)
    albedo = rng.uniform(-0.1, 1.1, (len(m["vertices"]), 3)).astype(np.float32)
    path = str(tmp_path / "a.ply")
    save_ply(path, {"vertices": m["vertices"], "faces": m["triangles"]})
    got = mr.read_ply(path)
    assert sorted(got) == ["faces", "x", "y", "z"] and got["x"].dtype == np.float32
    assert np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1), m["vertices"]) and np.array_equal(got["faces"], m["triangles"])
    utm = m["vertices"].astype(np.float64) * np.array([300.0, 300.0, 60.0]) + np.array([436000.25, 3355000.5, 20.0])
    save_ply(path, {"vertices": m["vertices"], "faces": m["triangles"], "normals": normals, "albedo": albedo, "vertices_utm": utm})
    got = mr.read_ply(path)
    assert got["x"].dtype == np.float64 and np.array_equal(np.stack([got["x"], got["y"], got["z"]], 1), utm)
    assert np.array_equal(np.stack([got["nx"], got["ny"], got["nz"]], 1), normals)
    assert np.array_equal(np.stack([got["red"], got["green"], got["blue"]], 1), np.rint(np.clip(albedo.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    assert np.array_equal(got["faces"], m["triangles"])
    assert level_from_opacity(0.5, 2 / 128) == pytest.approx(np.log(2.0) * 64, rel=1e-15)
    with pytest.raises(ValueError):
        level_from_opacity(1.0, 0.1)
