"""The holders of csrc/smpc_own.h (DevBuf, PinnedBuf, Event, Stream) on the CPU: tests/own_check/main.cpp
defines counting stand-ins for the eight runtime calls they make and checks moves, ensure's three
cases, a failed allocation, release() and that nothing is live at exit.  Built with a plain g++ under
AddressSanitizer and UBSan and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_the_holders_free_what_they_hold_once(tmp_path):
    exe = tmp_path / "own_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", os.path.join(ROOT, "tests", "own_check", "main.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
