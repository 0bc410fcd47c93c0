"""The plan of pe_place_best_fit_domains (csrc/pe_best_fit_plan.h) on the CPU: tests/cpp/test_best_fit_plan.cc, a
stand-alone program compiled here with the address and undefined-behaviour sanitizers and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_best_fit_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_best_fit_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_best_fit_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "60 plans, 5 refusals, 0 failures" in p.stdout, p.stdout + p.stderr
    assert "FAIL" not in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
