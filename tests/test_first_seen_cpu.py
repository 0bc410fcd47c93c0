"""The first-seen dedupe of the gang-capacity calls (csrc/pe_first_seen.h) on the CPU:
tests/cpp/test_first_seen.cc is a stand-alone program, compiled here with the address and
undefined-behaviour sanitizers and run directly.  It checks every item's number and the order of the
distinct keys against a brute-force scan -- equal, distinct, run-length, recurring and colliding keys, at
the table's smallest sizes and a few thousand items -- the predecessor shortcut, and a smaller call on the
storage of a larger one."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_first_seen.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_first_seen_matches_brute_force(tmp_path):
    exe = tmp_path / "test_first_seen"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) cases, (\d+) items checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 40000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
