"""The plan of pe_drain_fit_domains (csrc/pe_drain_plan.h) on the CPU: tests/cpp/test_drain_plan.cc is a stand-alone
program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It checks every
candidate's slot list, its runs and the synthetic jobs against a brute force on 300 random books, plans by hand for
candidates with 0 pods, 1 pod and every pod of the call, counts of 2^31 - 1, and every refusal with its index, each
leaving the plan as it was.  (The refusal of more than 2^31 - 1 pod slots needs a pod_node of 8 GiB and is not run.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_drain_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_drain_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_drain_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) plans, (\d+) slots, (\d+) runs checked, (\d+) refusals, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 2000 and int(m.group(3)) > 1000 and int(m.group(4)) >= 20
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
