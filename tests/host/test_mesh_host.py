"""CPU: the refusals of the mesh entry points in their documented order, the 64-bit size arithmetic at EONERF_MESH_MAX_POINTS and one
beyond, the workspace carve and the rule's per-point functions (csrc/eonerf_mesh_check.h, what the entry points and kernels of
include/eonerf_mesh.h call), checked by the stand-alone program tests/host/mesh_checks.cpp built host-only under the address and
undefined-behaviour sanitizers, exactly as tests/host/test_normals_host.py builds normals_checks.cpp, and run as a program.  The same
program meshes volumes from a file: its output is compared bit for bit with the numpy restatement (tests/mesh_restated.py)."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_restated as mr  # noqa: E402
import sanitized  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("mesh_host") / "mesh_checks", "mesh_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "mesh checks ok", args)


def test_mesh_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def volumes():
    rng = np.random.default_rng(11)
    yield "random 6x5x4", rng.standard_normal((4, 5, 6)).astype(np.float32), 0.1, (0.5, -2.0, 3.0), (0.25, 0.5, -1.5)
    f = rng.standard_normal((3, 4, 5)).astype(np.float32)
    f.reshape(-1)[[3, 17, 31, 44]] = [np.nan, np.inf, -np.inf, 0.25]
    f.reshape(-1)[[8, 9]] = [3e38, -3e38]            # both differences overflow on the edge between them: a NaN quotient
    yield "not finite, values on the level", f, 0.25, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    yield "overflowing differences", f, -2e38, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    big = np.full((2, 3, 700), -1.0, dtype=np.float32)          # 4200 points: five scan tiles
    big[:, :, ::7] = 1.0
    yield "across scan tiles", big, 0.0, (-1.0, -1.0, -1.0), (1 / 350, 1.0, 2.0)


def test_host_run_of_the_kernels_rule_equals_the_restatement_bit_for_bit(exe, tmp_path):
    for name, f, level, origin, spacing in volumes():
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        nz, ny, nx = f.shape
        with open(src, "wb") as fh:
            fh.write(struct.pack("<3i7f", nx, ny, nz, level, *origin, *spacing) + f.tobytes())
        run(exe, [src, dst])
        raw = open(dst, "rb").read()
        nv, nt, nonfinite = struct.unpack_from("<3q", raw)
        vertices = np.frombuffer(raw, np.float32, nv * 3, 24).reshape(nv, 3)
        keys = np.frombuffer(raw, np.int64, nv, 24 + 12 * nv)
        triangles = np.frombuffer(raw, np.int32, nt * 3, 24 + 20 * nv).reshape(nt, 3)
        want = mr.extract(f, level, origin, spacing)
        assert (nv, nt, nonfinite) == (len(want["keys"]), len(want["triangles"]), want["nonfinite"]), name
        assert nv > 0 and nt > 0, name
        assert np.array_equal(keys, want["keys"]), name
        assert vertices.tobytes() == want["vertices"].tobytes(), name
        assert np.array_equal(mr.rotate_smallest_first(triangles), mr.rotate_smallest_first(want["triangles"])), name
