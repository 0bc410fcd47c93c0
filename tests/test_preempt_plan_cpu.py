"""The plan of pe_gang_preempt_domains (csrc/pe_preempt_plan.h) on the CPU: tests/cpp/test_preempt_plan.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It checks
the release records, the victim -> record CSR, the pairs' lists in plan order and the per-node sums against a brute
force on the named hierarchies and 300 random inputs, merged runs and -1 slots, a plan by hand, the saturated
products, and that every refusal leaves the plan as it was."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_preempt_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_preempt_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_preempt_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) plans, (\d+) records, (\d+) lists, (\d+) sums checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 10000 and int(m.group(3)) > 10000 and int(m.group(4)) > 10000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_unit_size_is_smaller_than_the_fit_calls():
    text = open(os.path.join(INC, "pe_preempt_plan.h")).read()
    m = re.search(r"constexpr int PRE_UNIT_PAIRS = (\d+);", text)
    fit = re.search(r"constexpr int FIT_UNIT_PAIRS = (\d+);", open(os.path.join(INC, "pe_fit_plan.h")).read())
    assert m and fit and 1 <= int(m.group(1)) < int(fit.group(1))
