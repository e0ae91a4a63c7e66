"""CPU: the refusals of eonerf_render_origin_grad and its 64-bit size arithmetic (csrc/eonerf_pose_check.h, the host functions the entry
point of include/eonerf_pose.h calls first), checked by the stand-alone program tests/host/pose_checks.cpp built host-only under the
address and undefined-behaviour sanitizers, exactly as tests/host/test_ortho_host.py builds pose_checks.cpp, and run as a program."""
import sanitized


def test_pose_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "pose_checks", "pose_checks.cpp"), "pose checks ok")
