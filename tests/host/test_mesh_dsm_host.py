"""CPU: the refusals of the mesh-DSM entry points in their documented order, the 64-bit arithmetic at the limits of the fixed-point range
(coordinates at +-2^29 and one beyond), the floor-division box with negative coordinates and the rule's per-sample functions
(csrc/eonerf_mesh_dsm_check.h, what the entry points and kernels of include/eonerf_mesh_dsm.h call), checked by the stand-alone program
tests/host/mesh_dsm_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/host/test_mesh_host.py builds mesh_checks.cpp, and run as a program.  The same program rasterises meshes from a file: its dsm, face
and counts are compared bit for bit with the numpy restatement (tests/mesh_dsm_restated.py) on the cases of tests/mesh_dsm_cases.py."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_dsm_cases as mc  # noqa: E402
import mesh_dsm_restated as md  # noqa: E402
import mesh_restated as mr  # noqa: E402
import sanitized  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("mesh_dsm_host") / "mesh_dsm_checks", "mesh_dsm_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "mesh dsm checks ok", args)


def test_mesh_dsm_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def all_cases():
    yield from mc.cases()
    f, level, origin, spacing = mc.sphere_volume()
    m = mr.extract(f, level, origin, spacing)
    yield mc.case("sphere 9^3 45x43", m["vertices"], m["triangles"], mc.SPHERE_GRID, mc.SPHERE_SCALE, mc.SPHERE_OFFSET)
    perm = np.random.default_rng(3).permutation(len(m["triangles"]))
    yield mc.case("sphere 9^3 permuted 45x43", m["vertices"], m["triangles"][perm], mc.SPHERE_GRID, mc.SPHERE_SCALE, mc.SPHERE_OFFSET)


def test_host_run_of_the_kernels_rule_equals_the_restatement_bit_for_bit(exe, tmp_path):
    sphere = []
    for c in all_cases():
        name = c["name"]
        xoff, yoff, xsize, ysize, res = c["grid"]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("<2q2i9d", len(c["vertices"]), len(c["triangles"]), xsize, ysize, *c["scale"], *c["offset"], xoff, yoff, res))
            fh.write(c["vertices"].tobytes() + c["triangles"].tobytes())
        run(exe, [src, dst])
        raw = open(dst, "rb").read()
        n = xsize * ysize
        assert len(raw) == 32 + 8 * n, name
        counts = np.frombuffer(raw, np.int64, 4)
        dsm = np.frombuffer(raw, np.float32, n, 32).reshape(ysize, xsize)
        face = np.frombuffer(raw, np.int32, n, 32 + 4 * n).reshape(ysize, xsize)
        want = md.rasterize(c["vertices"], c["triangles"], c["scale"], c["offset"], xoff, yoff, xsize, ysize, res)
        assert counts.tolist() == want["counts"].tolist(), (name, counts.tolist(), want["counts"].tolist())
        assert dsm.tobytes() == want["dsm"].tobytes(), name
        assert face.tobytes() == want["face"].tobytes(), name
        assert counts[:3].sum() == len(c["triangles"]), name
        if name.startswith("sphere"):
            sphere.append(dsm.tobytes())
    assert len(sphere) == 2 and sphere[0] == sphere[1]
