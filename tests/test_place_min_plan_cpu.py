"""The plan of pe_place_min_member_domains (csrc/pe_place_min_plan.h) on the CPU: tests/cpp/test_place_min_plan.cc
is a stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It
checks every group's mandatory and optional share and the records built from them against a walk over the pod
slots on 400 random batches, min_member at 0, -1, T and 2^31 - 1 with counts of 2^31 - 1, each refusal with its
index, and that a refusal leaves the plan as it was."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_place_min_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_place_min_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_place_min_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) plans, (\d+) jobs, (\d+) groups checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 400 and int(m.group(2)) > 5000 and int(m.group(3)) > 10000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
