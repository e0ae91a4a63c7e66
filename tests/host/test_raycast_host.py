"""CPU: the refusals of the ray casting entry points in their documented order, the 64-bit size arithmetic at the limits (2^27 cells,
2^31 - 1 entries, the strides), the padded cell range with negative and boundary coordinates, the stepper with zero direction
components and the rule's per-ray functions (csrc/eonerf_raycast_check.h, what the entry points and kernels of csrc/eonerf_raycast.h
call), checked by the stand-alone program tests/host/raycast_checks.cpp built host-only under the address and undefined-behaviour
sanitizers, exactly as tests/host/test_smooth_host.py builds smooth_checks.cpp, and run as a program.  The same program casts rays
through the GRID from a file: t, face, bary, the occluded bytes and the counts are compared bit for bit with the brute-force
restatement (tests/raycast_restated.py) on every case of tests/raycast_cases.py that is not big."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import raycast_cases as rcc  # noqa: E402
import raycast_restated as rc  # noqa: E402
import sanitized  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("raycast_host") / "raycast_checks", "raycast_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "raycast checks ok", args)


def test_raycast_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_host_run_of_the_grid_equals_the_brute_force_bit_for_bit(exe, tmp_path):
    done = 0
    for c in rcc.cases():
        if c["big"]:
            continue
        name = c["name"]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        n_v, n_t, n = len(c["vertices"]), len(c["triangles"]), len(c["origins"])
        with open(src, "wb") as fh:
            fh.write(struct.pack("<3q4i8d", n_v, n_t, n, *c["dims"], int(c["skip"] is not None), *c["lo"].tolist(), *c["hi"].tolist(), c["t_min"], c["t_max"]))
            fh.write(c["vertices"].tobytes() + c["triangles"].tobytes() + c["origins"].tobytes() + c["dirs"].tobytes())
            if c["skip"] is not None:
                fh.write(c["skip"].tobytes())
        run(exe, [src, dst])
        raw = open(dst, "rb").read()
        assert len(raw) == 64 + n * (8 + 4 + 12 + 1), name
        head = np.frombuffer(raw, np.int64, 8)
        at = 64
        t = np.frombuffer(raw, np.float64, n, at); at += 8 * n
        face = np.frombuffer(raw, np.int32, n, at); at += 4 * n
        bary = np.frombuffer(raw, np.float32, 3 * n, at).reshape(n, 3); at += 12 * n
        occ = np.frombuffer(raw, np.uint8, n, at)
        want = rc.closest(c["vertices"], c["triangles"], c["lo"], c["hi"], c["origins"], c["dirs"], c["t_min"], c["t_max"])
        block = rc.occluded(c["vertices"], c["triangles"], c["lo"], c["hi"], c["origins"], c["dirs"], c["skip"], c["t_min"], c["t_max"])
        entries = rc.cell_entries(c["vertices"], c["triangles"], c["lo"], c["hi"], c["dims"])[1]
        assert head.tolist() == [entries, want["dropped"], *want["counts"].tolist(), *block["counts"].tolist()], (name, head.tolist())
        bad = np.nonzero((face != want["face"]) | (t.view(np.int64) != want["t"].view(np.int64)))[0]
        assert not len(bad), (name, len(bad), bad[:5].tolist(), t[bad[:5]].tolist(), want["t"][bad[:5]].tolist(), face[bad[:5]].tolist(), want["face"][bad[:5]].tolist())
        assert same_bits(bary, want["bary"]), name
        assert same_bits(occ, block["occluded"]), (name, np.nonzero(occ != block["occluded"])[0][:5].tolist())
        done += 1
    assert done >= 25
