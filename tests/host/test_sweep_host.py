"""CPU: the sun sweep's workspace layout (carve_sweep, csrc/eonerf_carve.h) and its 64-bit ray bound, checked by the stand-alone
program tests/host/sweep_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/test_host_sanitizers.py builds host_checks.cpp, and run as a program."""
import sanitized


def test_carve_sweep_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "sweep_checks", "sweep_checks.cpp"), "sweep checks ok")
