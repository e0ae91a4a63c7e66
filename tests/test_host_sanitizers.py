"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer build of the C ABI's HOST logic (GPU sanitizers are not available on
this pool): the parameter layout and packed-stream gather maps of csrc/eonerf_pack.cpp and the workspace carving of csrc/eonerf_carve.h,
driven by tests/host/host_checks.cpp.  Compiled host-only with the ROCm clang (the sources share headers with the device code)."""
import os
import sys

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "host"))

import sanitized  # noqa: E402


def test_pack_and_carve_host_logic_under_asan_ubsan(tmp_path):
    sanitized.run(sanitized.build(tmp_path / "host_checks", "host_checks.cpp", sanitized.PACK), "host checks ok")
