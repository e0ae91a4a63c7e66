"""CPU: the refusals of the component entry points in their documented order, the 64-bit size arithmetic at EONERF_MESH_MAX_POINTS and
one beyond, and the rule's predicates (csrc/eonerf_components_check.h, what the entry points and kernels of
include/eonerf_components.h call), checked by the stand-alone program tests/host/components_checks.cpp built host-only under the address
and undefined-behaviour sanitizers, exactly as tests/host/test_mesh_host.py builds mesh_checks.cpp, and run as a program.  The same
program labels and filters volumes from a file with a plain sequential union-find over those predicates: its output is compared bit
for bit with the numpy restatement (tests/components_restated.py)."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import components_restated as cr  # noqa: E402
import sanitized  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("components_host") / "components_checks", "components_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "components checks ok", args)


def test_components_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def volumes():
    rng = np.random.default_rng(31)
    yield "random 6x5x4", rng.standard_normal((4, 5, 6)).astype(np.float32), 0.1, 3, 0
    f = rng.standard_normal((3, 4, 5)).astype(np.float32)
    f.reshape(-1)[[3, 17, 31, 44, 45]] = [np.nan, np.inf, -np.inf, 0.25, 0.25]
    yield "not finite, values on the level", f, 0.25, 2, 1
    yield "sparse 40x9x5", (rng.random((5, 9, 40)) < 0.2).astype(np.float32), 0.5, 4, 0
    yield "dense 40x9x5", (rng.random((5, 9, 40)) < 0.6).astype(np.float32), 0.5, 10, 1


def test_host_union_find_equals_the_restatement_bit_for_bit(exe, tmp_path):
    for name, f, level, min_points, protect in volumes():
        for side in (0, 1):
            protect = 1 if side else protect
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            nz, ny, nx = f.shape
            with open(src, "wb") as fh:
                fh.write(struct.pack("<4if", nx, ny, nz, side, level) + f.tobytes() + struct.pack("<qi", min_points, protect))
            run(exe, [src, dst])
            raw = open(dst, "rb").read()
            n = f.size
            assert len(raw) == 48 + 12 * n
            counts, dropped = struct.unpack_from("<4q", raw), struct.unpack_from("<2q", raw, 32)
            labels = np.frombuffer(raw, np.int32, n, 48).reshape(f.shape)
            info = np.frombuffer(raw, np.uint32, n, 48 + 4 * n).reshape(f.shape)
            f_out = np.frombuffer(raw, np.float32, n, 48 + 8 * n).reshape(f.shape)
            want = cr.label(f, level, side)
            assert counts == want["counts"] and counts[0] > 0, (name, side, counts, want["counts"])
            assert labels.tobytes() == want["labels"].tobytes(), (name, side)
            assert info.tobytes() == want["info"].tobytes(), (name, side)
            want_out, want_dropped = cr.filter_volume(f, want["labels"], want["info"], side, min_points, protect)
            assert dropped == want_dropped, (name, side, dropped, want_dropped)
            assert f_out.tobytes() == want_out.tobytes(), (name, side)
