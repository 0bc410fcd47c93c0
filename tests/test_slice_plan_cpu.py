"""The host side of pe_gang_slice_tree (csrc/pe_slice_plan.h) on the CPU: tests/cpp/test_slice_plan.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It
checks each refusal with its first offending index, the dedupe into rows and picks and the canonical row of z = 1
against a brute-force scan on 400 random batches, and the unit conversion at 0, z - 1, z, PE_CAP_MAX and
z = 2^31 - 1."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_slice_plan.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_slice_plan_matches_brute_force(tmp_path):
    exe = tmp_path / "test_slice_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) batches, (\d+) jobs checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 10000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
