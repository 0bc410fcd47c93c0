"""The plan of pe_place_first_fit_domains (csrc/pe_first_fit_plan.h) on the CPU: tests/cpp/test_first_fit_plan.cc is
a stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It checks
the ranks, the jobs' candidate lists and the domains' queues against a brute force on the named hierarchies and 300
random maps and lists, equal priorities, jobs in no pair, repeated pairs, a plan worked by hand, and that every
refusal leaves the plan as it was."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_first_fit_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_first_fit_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_first_fit_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) plans, (\d+) pairs, (\d+) queues checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 5000 and int(m.group(3)) > 1000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
