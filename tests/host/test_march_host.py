"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer build of the march's HOST logic -- the workspace layout behind
eonerf_march_workspace_bytes (carve_march, csrc/eonerf_carve.h), the refusal order of eonerf_render_forward_march (march_refusal) and
the recorded sizes of carve_render -- driven by the stand-alone tests/host/march_checks.cpp.  Compiled host-only, the way
tests/host/test_occ_host.py compiles occ_checks.cpp, and run as a program."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HIPCC = "/opt/rocm/bin/hipcc"


def test_march_layout_and_refusals_host_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "march_checks")
    # host-only instrumentation: -fno-gpu-sanitize keeps the sanitizers off every device compilation, whatever the driver decides
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", os.path.join(REPO, "tests", "host", "march_checks.cpp"),
           os.path.join(REPO, "eonerf_code_amd", "csrc", "eonerf_pack.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "march host checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
