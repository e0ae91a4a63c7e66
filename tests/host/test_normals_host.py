"""CPU: the refusals of eonerf_field_density_grad / eonerf_render_normals in their documented order and the 64-bit size arithmetic
(csrc/eonerf_normals_check.h, the host functions the entry points of include/eonerf_normals.h call first), checked by the stand-alone
program tests/host/normals_checks.cpp built host-only under the address and undefined-behaviour sanitizers, exactly as
tests/host/test_pose_host.py builds pose_checks.cpp, and run as a program."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HIPCC = "/opt/rocm/bin/hipcc"


def test_normals_host_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "normals_checks")
    # host-only instrumentation: -fno-gpu-sanitize keeps the sanitizers off every device compilation, whatever the driver decides
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", os.path.join(REPO, "tests", "host", "normals_checks.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "normals checks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
