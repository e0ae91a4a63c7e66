"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer build of the march's HOST logic -- the workspace layout behind
eonerf_march_workspace_bytes (carve_march, csrc/eonerf_carve.h), the refusal order of eonerf_render_forward_march (march_refusal) and
the recorded sizes of carve_render -- driven by the stand-alone tests/host/march_checks.cpp.  Compiled host-only, the way
tests/host/test_occ_host.py compiles occ_checks.cpp, and run as a program."""
import sanitized


def test_march_layout_and_refusals_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "march_checks", "march_checks.cpp", sanitized.PACK), "march host checks ok")
