"""CPU: the refusals of the simplification entry points in their documented order, the 64-bit size arithmetic at the limits (dims of
4096, 2^27 cells, 2^31 - 1 vertices and triangles), the clamp at both grid borders, ties-to-even at x.5 sub-cells and the rule's
per-vertex and per-triangle functions (csrc/eonerf_simplify_check.h, what the entry points and kernels of csrc/eonerf_simplify.h call),
checked by the stand-alone program tests/host/simplify_checks.cpp built host-only under the address and undefined-behaviour sanitizers,
exactly as tests/host/test_mesh_dsm_host.py builds mesh_dsm_checks.cpp, and run as a program.  The same program simplifies meshes from
a file: its vertices, source, vertex_map, triangles and counts are compared bit for bit with the numpy restatement
(tests/simplify_restated.py) on the cases of tests/simplify_cases.py, in both modes."""
import os
import struct
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sanitized  # noqa: E402
import simplify_cases as sc  # noqa: E402
import simplify_restated as sr  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("simplify_host") / "simplify_checks", "simplify_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "simplify checks ok", args)


def test_simplify_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def test_host_run_of_the_kernels_rule_equals_the_restatement_bit_for_bit(exe, tmp_path):
    done = 0
    for c in sc.cases():
        if c["big"]:
            continue
        for representative in (sr.MEAN, sr.NEAREST):
            name = (c["name"], representative)
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            n_v, n_t = len(c["vertices"]), len(c["triangles"])
            with open(src, "wb") as fh:
                fh.write(struct.pack("<2q4i6f", n_v, n_t, *c["dims"], representative, *c["origin"].tolist(), *c["cell"].tolist()))
                fh.write(c["vertices"].tobytes() + c["triangles"].tobytes())
            run(exe, [src, dst])
            raw = open(dst, "rb").read()
            want = sr.simplify(c["vertices"], c["triangles"], c["origin"], c["cell"], c["dims"], representative)
            counts = np.frombuffer(raw, np.int64, 4)
            assert counts.tolist() == want["counts"].tolist(), (name, counts.tolist(), want["counts"].tolist())
            n_out, kept = int(counts[0]), int(counts[1])
            assert len(raw) == 32 + 16 * n_out + 4 * n_v + 12 * kept, name
            at = 32
            assert raw[at:at + 12 * n_out] == want["vertices"].tobytes(), name
            at += 12 * n_out
            assert raw[at:at + 4 * n_out] == want["source"].tobytes(), name
            at += 4 * n_out
            assert raw[at:at + 4 * n_v] == want["vertex_map"].tobytes(), name
            at += 4 * n_v
            assert raw[at:] == want["triangles"].tobytes(), name
            assert counts[1:].sum() == n_t, name
            done += 1
    assert done >= 40
