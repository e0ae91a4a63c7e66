"""CPU: the refusals of the dual-contouring entry points in their documented order, the 64-bit size arithmetic at
EONERF_MESH_MAX_POINTS and one beyond, the workspace carve and the rule's per-element functions (csrc/eonerf_dual_check.h, what the
entry points and kernels of csrc/eonerf_dual.h call), checked by the stand-alone program tests/host/dual_checks.cpp built host-only
under the address and undefined-behaviour sanitizers through tests/host/sanitized.py, and run as a program.  The same program contours
every case of tests/dual_cases.py that is not big: its output is compared bit for bit with the numpy restatement
(tests/dual_restated.py), vertices included."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dual_cases as dc  # noqa: E402
import dual_restated as dr  # noqa: E402
import sanitized  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("dual_host") / "dual_checks", "dual_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "dual checks ok", args)


def test_dual_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def host_contour(exe, tmp_path, case):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    nz, ny, nx = case["f"].shape
    with open(src, "wb") as fh:
        fh.write(struct.pack("<3i8fq", nx, ny, nz, case["level"], *case["origin"], *case["spacing"], case["lam"], len(case["g"])))
        fh.write(case["f"].tobytes() + case["g"].tobytes())
    run(exe, [src, dst])
    raw = open(dst, "rb").read()
    head = struct.unpack_from("<8q", raw)
    n_h, n_v, n_t = head[:3]
    at = 64
    out = {"head": head}
    for name, dtype, shape in (("points", np.float32, (n_h, 3)), ("keys", np.int64, (n_h,)), ("vertices", np.float32, (n_v, 3)),
                               ("cell_keys", np.int64, (n_v,)), ("triangles", np.int32, (n_t, 3))):
        count = int(np.prod(shape))
        out[name] = np.frombuffer(raw, dtype, count, at).reshape(shape)
        at += count * np.dtype(dtype).itemsize
    assert at == len(raw)
    return out


def test_host_run_of_the_kernels_rule_equals_the_restatement_bit_for_bit(exe, tmp_path):
    seen = 0
    for case in dc.cases(big=False):
        name = case["name"]
        got = host_contour(exe, tmp_path, case)
        want = dr.contour(case["f"], case["level"], case["g"], case["origin"], case["spacing"], case["lam"])
        assert got["head"] == dr.counts_of(want) + want["report"][:3] + (0,), (name, got["head"])
        for key in ("keys", "points", "cell_keys", "vertices", "triangles"):         # triangles in the rule's own order and rotation
            assert dc.same_bits(got[key], want[key]), (name, key)
        seen += 1
    assert seen >= 17
