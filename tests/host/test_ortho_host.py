"""CPU: the true orthophoto's refusals and its 64-bit size arithmetic (csrc/eonerf_ortho_check.h, the host functions the entry points of
include/eonerf_ortho.h call first), checked by the stand-alone program tests/host/ortho_checks.cpp built host-only under the address
and undefined-behaviour sanitizers, exactly as tests/host/test_sweep_host.py builds sweep_checks.cpp, and run as a program."""
import sanitized


def test_ortho_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "ortho_checks", "ortho_checks.cpp"), "ortho checks ok")
