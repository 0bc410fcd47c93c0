"""The reciprocal division of the gang-capacity kernel (csrc/pe_divmagic.h) against unsigned __int128
division on the CPU: tests/cpp/test_divmagic.cc is a stand-alone program, compiled here with the
address and undefined-behaviour sanitizers and run directly."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_divmagic.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_divmagic_matches_int128_division(tmp_path):
    exe = tmp_path / "test_divmagic"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) divisors, (\d+) checks, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 3204 and int(m.group(2)) > 300_000
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
