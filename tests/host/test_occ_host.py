"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer build of the occupancy grid's HOST logic -- the workspace layout behind
eonerf_occ_workspace_bytes (carve_occ, csrc/eonerf_carve.h) and the fact that a grid set on a context moves nothing in the layouts of
eonerf_render_forward and eonerf_render_sun_sweep -- driven by the stand-alone tests/host/occ_checks.cpp.  Compiled host-only, the way
tests/test_host_sanitizers.py compiles host_checks.cpp, and run as a program."""
import sanitized


def test_occ_workspace_layout_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "occ_checks", "occ_checks.cpp", sanitized.PACK), "occ host checks ok")
