"""The host plan of pe_fit_explain (csrc/pe_explain_plan.h) on the CPU: tests/cpp/test_explain_plan.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It checks
that the chunks cover [0, S) exactly at budgets giving chunks of 1, S - 1, S and S + 1 records, the leaf ->
level-domain map against a brute-force walk on random hierarchies of 1 to 4 levels with -1 parents, every refusal
with its first offending index, and the dedupe against a brute-force scan: equal shapes in different domains stay
distinct."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_explain_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_explain_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_explain_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) cases, (\d+) checks, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 500 and int(m.group(2)) > 40000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
