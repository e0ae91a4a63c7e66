"""CPU: the refusals of eonerf_field_density_grad / eonerf_render_normals in their documented order and the 64-bit size arithmetic
(csrc/eonerf_normals_check.h, the host functions the entry points of include/eonerf_normals.h call first), checked by the stand-alone
program tests/host/normals_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/host/test_pose_host.py builds pose_checks.cpp, and run as a program."""
import sanitized


def test_normals_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "normals_checks", "normals_checks.cpp"), "normals checks ok")
