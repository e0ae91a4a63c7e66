"""CPU: the component rule as restated in numpy (tests/components_restated.py) -- against scipy.ndimage.label with the 15-voxel
structure of the seven directions, against the mesh restatement (every triangle in one component; dropping a component is filtering
the mesh), on a hollow sphere -- and the binding's symbol list against the new header.  The device tests
(tests/test_components_gpu.py) compare the library with this restatement bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest

import components_restated as cr
import mesh_restated as mr
from conftest import REPO

SHAPES = [(11, 10, 9), (3, 4, 5), (33, 9, 17)]          # (nz, ny, nx) of the 9x10x11, 5x4x3 and 17x9x33 volumes


def test_restatement_imports_nothing_but_numpy():
    src = open(os.path.join(REPO, "tests", "components_restated.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", src, flags=re.M) == ["numpy"]


# ---- header pins ------------------------------------------------------------------------------------------------------------------
def test_components_header_symbols_are_bound_and_exported():
    from eonerf_code_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(REPO, "include", "eonerf_components.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.eonerf_cc_version.restype = ctypes.c_int
    assert L.eonerf_cc_version() == 1
    assert int(re.search(r"#define\s+EONERF_CC_VERSION\s+(\d+)", hdr).group(1)) == 1
    for axis in "XYZ":
        assert int(re.search(r"#define\s+EONERF_CC_TILE_%s\s+(\d+)" % axis, hdr).group(1)) >= 2
    L.eonerf_version.restype = ctypes.c_int
    assert L.eonerf_version() == 502
    L.eonerf_mesh_version.restype = ctypes.c_int
    assert L.eonerf_mesh_version() == 1
    L.eonerf_cc_workspace_bytes.restype = ctypes.c_size_t
    wb = L.eonerf_cc_workspace_bytes
    assert wb(1, 2, 2) == 0 and wb(2, 2, 1) == 0 and wb((1 << 14) + 1, 1 << 13, 2) == 0 and wb(1 << 16, 1 << 16, 1 << 16) == 0
    assert wb(2, 2, 2) > 0 and wb(1 << 14, 1 << 13, 2) > 0


# ---- against scipy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.05, 0.15, 0.2, 0.5])
def test_restatement_agrees_with_scipy_on_the_14_neighbourhood(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = cr.structure14()
    assert structure.sum() == 15 and not structure[1, 0, 2] and not structure[1, 2, 0] and structure[1, 2, 2] and structure[2, 2, 2]
    f = (np.random.default_rng(1).random((17, 33, 129)) < density).astype(np.float32)
    for side in (0, 1):
        got = cr.label(f, 0.5, side)
        ref, n_ref = ndimage.label(cr.side_mask(f, 0.5, side), structure=structure)
        assert got["counts"][0] == n_ref and n_ref > 0
        assert cr.same_partition((got["labels"], -1), (ref, 0))
        flat = got["labels"].reshape(-1)
        roots = np.unique(flat[flat >= 0])
        assert (flat[roots] == roots).all() and len(roots) == n_ref                  # a label is a point of its own component ...
        first = np.full(flat.size, flat.size, dtype=np.int64)
        np.minimum.at(first, flat[flat >= 0], np.nonzero(flat >= 0)[0])
        assert (first[roots] == roots).all()                                         # ... the one with the smallest index
        size = np.bincount(ref.reshape(-1))[1:]
        assert got["counts"][1] == int(size.sum()) and got["counts"][2] == int(size.max())
        assert sorted((got["info"].reshape(-1)[roots] & 0x7FFFFFFF).tolist()) == sorted(size.tolist())


def test_anisotropy_of_one_cell():
    f = np.full((2, 2, 2), -1.0, dtype=np.float32)
    f[0, 0, 0] = f[0, 1, 1] = 1.0                       # 000 and 110: an edge of the split
    assert cr.label(f, 0.0)["counts"] == (1, 2, 2, 0)
    f = np.full((2, 2, 2), -1.0, dtype=np.float32)
    f[0, 0, 1] = f[0, 1, 0] = 1.0                       # 100 and 010: no edge
    assert cr.label(f, 0.0)["counts"] == (2, 2, 1, 1)
    assert cr.label(f, 0.0, 1)["counts"] == (1, 6, 6, 0)


# ---- the two mesh properties ------------------------------------------------------------------------------------------------------
def submesh(mesh, keep):
    """The mesh without the vertices where `keep` is false and without every triangle that names one; ids renumbered by a prefix sum."""
    new_id = np.cumsum(keep) - 1
    tri = mesh["triangles"]
    tri_keep = keep[tri].all(axis=1)
    assert (keep[tri].any(axis=1) == tri_keep).all()                                 # a triangle is dropped whole or not at all
    return {"vertices": mesh["vertices"][keep], "keys": mesh["keys"][keep], "triangles": new_id[tri[tri_keep]].astype(np.int32)}


def volume_with(shape, side, want):
    """The first seeded random volume of `shape` on which the filter of `side` has something to drop and something to keep."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        f = (rng.standard_normal(shape) + (0.0 if side == 0 else 0.9)).astype(np.float32)
        lab = cr.label(f, 0.0, side)
        roots = cr.dropped_roots(lab["info"], *want(lab))
        if 0 < len(roots) < lab["counts"][0]:
            return f, lab
    raise AssertionError(f"no seed gives {shape} a component to drop on side {side}")


@pytest.mark.parametrize("side", [0, 1], ids=["drop to -inf", "fill to +inf"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(d) for d in s[::-1]))
def test_every_triangle_has_one_component_and_dropping_it_filters_the_mesh(shape, side):
    # side 0: everything below the largest component goes; side 1: every outside component off the boundary (a cavity) is filled
    want = (lambda lab: (lab["counts"][2], False)) if side == 0 else (lambda lab: (1 << 29, True))
    f, lab = volume_with(shape, side, want)
    min_points, protect = want(lab)
    mesh = mr.extract(f, 0.0, (-1.0, 0.5, 2.0), (0.5, 0.25, 2.0))
    comp = cr.vertex_components(mesh["keys"], lab["labels"], shape)
    assert (comp >= 0).all() and len(mesh["triangles"]) > 0
    per_triangle = comp[mesh["triangles"]]
    assert (per_triangle == per_triangle[:, :1]).all()
    f_out, (n_comp, n_points) = cr.filter_volume(f, lab["labels"], lab["info"], side, min_points, protect)
    roots = cr.dropped_roots(lab["info"], min_points, protect)
    assert n_comp == len(roots) > 0 and n_points == int((lab["info"].reshape(-1)[roots] & 0x7FFFFFFF).sum())
    changed = f_out.view(np.int32) != f.view(np.int32)
    assert (f_out[changed] == (np.inf if side else -np.inf)).all() and changed.sum() <= n_points
    got = mr.extract(f_out, 0.0, (-1.0, 0.5, 2.0), (0.5, 0.25, 2.0))
    expect = submesh(mesh, ~np.isin(comp, roots))
    assert got["nonfinite"] == 0 and len(expect["keys"]) < len(mesh["keys"])
    assert np.array_equal(got["keys"], expect["keys"])
    assert got["vertices"].tobytes() == expect["vertices"].tobytes()
    assert np.array_equal(got["triangles"], expect["triangles"])                     # the order too


# ---- a hollow sphere --------------------------------------------------------------------------------------------------------------
def hollow_sphere(n=17, outer=6.3, inner=3.2):
    c = (n - 1) / 2 + np.array([0.137, 0.187, -0.073])
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return np.minimum(outer - r, r - inner).astype(np.float32)


def test_fill_cavities_removes_exactly_the_inner_surface_of_a_hollow_sphere():
    f = hollow_sphere()
    inside, outside = cr.label(f, 0.0, 0), cr.label(f, 0.0, 1)
    assert inside["counts"][0] == 1 and outside["counts"][0] == 2
    flat = outside["info"].reshape(-1)
    roots = np.nonzero(flat)[0]
    cavity = [int(r) for r in roots if not flat[r] & cr.BOUNDARY]
    assert len(cavity) == 1 and outside["counts"][3] == 0                            # the world starts at point 0; the cavity is the other one
    mesh = mr.extract(f, 0.0)
    assert mr.euler_characteristic(len(mesh["vertices"]), mesh["triangles"]) == 4    # two spheres
    filled, (n_comp, n_points) = cr.filter_volume(f, outside["labels"], outside["info"], 1, 1 << 29, True)
    assert n_comp == 1 and n_points == int(flat[cavity[0]] & 0x7FFFFFFF)
    got = mr.extract(filled, 0.0)
    comp = cr.vertex_components(mesh["keys"], outside["labels"], f.shape)           # by the outside end: world or cavity
    expect = submesh(mesh, comp != cavity[0])
    assert np.array_equal(got["keys"], expect["keys"]) and got["vertices"].tobytes() == expect["vertices"].tobytes()
    assert np.array_equal(got["triangles"], expect["triangles"]) and got["nonfinite"] == 0
    assert 0 < len(got["triangles"]) < len(mesh["triangles"])
    most, unpaired = mr.edge_report(got["triangles"])
    assert most == 1 and len(unpaired) == 0
    assert mr.euler_characteristic(len(got["vertices"]), got["triangles"]) == 2
    assert mr.signed_volume(got["vertices"], got["triangles"]) > mr.signed_volume(mesh["vertices"], mesh["triangles"]) > 0
