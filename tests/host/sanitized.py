"""The one build line, environment and run-and-assert step of the host sanitizer tests (tests/host/test_*_host.py and
tests/test_host_sanitizers.py): a stand-alone C++ program over the library's HOST logic, compiled host-only with the ROCm clang (the
sources share headers with the device code) under the address and undefined-behaviour sanitizers, and run as a program.  It lives in
tests/host/ because that directory stays on the CPU machine."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = "/opt/rocm/bin/hipcc"
PACK = os.path.join(REPO, "eonerf_code_amd", "csrc", "eonerf_pack.cpp")        # what four of the programs link besides their own source
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def build(exe, *sources):
    """Compile tests/host/<source> (or an absolute path) into the program `exe`; returns `exe`."""
    # host-only instrumentation: -fno-gpu-sanitize keeps the sanitizers off every device compilation, whatever the driver decides
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", *(os.path.join(REPO, "tests", "host", s) for s in sources),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    return str(exe)


def run(exe, ok, args=()):
    """Run the program: it ends with status 0, prints `ok`, and neither sanitizer reports anything."""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
