"""csrc/smpc_group_layout.h on the CPU: tests/group_check/main.cpp holds the layout of a group's arrays
to the formulas smpc_group_create used to compute inline (n in {1, 2, 16, 37}, a slot capacity that is
a multiple of 256 and one that is not), and the partition of a round into launches to cases written
out by hand (nobody eligible; lane members that agree, one alone, that disagree, past the LDS limit;
wave instances interleaved and alone; members not taken; the `dep` row).  Built with a plain g++ under
AddressSanitizer and UBSan and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_groups_layout_and_partition(tmp_path):
    exe = tmp_path / "group_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         os.path.join(ROOT, "tests", "group_check", "main.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr)
