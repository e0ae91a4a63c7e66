"""CPU: the refusals of the smoothing entry points in their documented order, the 64-bit size arithmetic at the limits (2^31 - 1
vertices, 2^29 triangles), rdiv on negative numerators and at |D| near 2^62, ties-to-even, the limit at both ends and the rule's
per-vertex functions (csrc/eonerf_smooth_check.h, what the entry points and kernels of csrc/eonerf_smooth.h call), checked by the
stand-alone program tests/host/smooth_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/host/test_simplify_host.py builds simplify_checks.cpp, and run as a program.  The same program smooths meshes from a file: its
vertices, counts and status are compared bit for bit with the numpy restatement (tests/smooth_restated.py) on every case of
tests/smooth_cases.py that is not big."""
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
import smooth_cases as sc  # noqa: E402
import smooth_restated as sm  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sanitized.build(tmp_path_factory.mktemp("smooth_host") / "smooth_checks", "smooth_checks.cpp")


def run(exe, args):
    sanitized.run(exe, "smooth checks ok", args)


def test_smooth_host_logic_under_asan_ubsan(exe):
    run(exe, [])


def test_host_run_of_the_kernels_rule_equals_the_restatement_bit_for_bit(exe, tmp_path):
    done = 0
    for c in sc.cases():
        if c["big"]:
            continue
        name = c["name"]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        n_v, n_t = len(c["vertices"]), len(c["triangles"])
        with open(src, "wb") as fh:
            fh.write(struct.pack("<2q4i6f", n_v, n_t, int(c["pin_open"]), int(c["pinned"] is not None), len(c["steps"]), 0, *c["origin"].tolist(), *c["unit"].tolist()))
            fh.write(np.asarray(c["steps"], dtype=np.int32).tobytes() + c["vertices"].tobytes() + c["triangles"].tobytes())
            if c["pinned"] is not None:
                fh.write(c["pinned"].tobytes())
        run(exe, [src, dst])
        raw = open(dst, "rb").read()
        want = sm.smooth(c["vertices"], c["triangles"], c["origin"], c["unit"], c["steps"], c["pinned"], c["pin_open"])
        counts = np.frombuffer(raw, np.int64, 6)
        assert counts.tolist() == want["counts"].tolist(), (name, counts.tolist(), want["counts"].tolist())
        assert len(raw) == 48 + 4 + 12 * n_v, name
        assert struct.unpack("<i", raw[48:52])[0] == want["status"], name
        assert raw[52:] == want["vertices"].tobytes(), name
        done += 1
    assert done >= 35
