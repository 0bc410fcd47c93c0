"""The plan of pe_release_gangs / pe_assume_gangs (csrc/pe_ledger_plan.h) on the CPU: tests/cpp/test_ledger_plan.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It checks
the touched nodes' new residuals, the counted pods, the steps and the refusal's node against a slot-by-slot brute
force on 300 random inputs with merged runs, -1 slots, removed slots and nodes repeated across gangs, a plan by hand,
100 000 pods on one node as one step, products and sums past int64, and that every refusal leaves the plan, its
scratch map and the outputs as they were."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ledger_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_ledger_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_ledger_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) plans, (\d+) slots, (\d+) nodes checked, (\d+) refusals, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 600 and int(m.group(2)) > 10000 and int(m.group(3)) > 1000 and int(m.group(4)) > 100
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_the_plan_header_needs_no_hip():
    for name in ("pe_ledger_plan.h", "pe_gang_slots.h"):
        text = open(os.path.join(INC, name)).read()
        assert "hip" not in re.sub(r"//[^\n]*", "", text).lower(), name
