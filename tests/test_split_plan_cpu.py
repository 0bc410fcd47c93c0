"""The host side of pe_gang_split_tree (csrc/pe_split_plan.h) on the CPU: tests/cpp/test_split_plan.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It
checks split_tr, the (t, r) arithmetic of the rule's threshold form, against a brute-force walk over sorted
children on 300 random child lists with ties and zeros (every allotment of each), at values near 2^55 and at a
count of 2^31 - 1; the slice sizes at the 64 MiB boundary; the copy ranges; the scatter from picks to jobs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_split_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_split_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_split_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) lists, (\d+) steps checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 3000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
