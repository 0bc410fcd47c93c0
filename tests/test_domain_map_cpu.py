"""What the domain calls' plans share (csrc/pe_domain_map.h) on the CPU: tests/cpp/test_domain_map.cc is a
stand-alone program, compiled here with the address and undefined-behaviour sanitizers and run directly.  It
checks the leaf -> level map, the numbering of the active domains and the deal of items to their domains against a
brute force on the named hierarchies and 300 random maps: level 0, the top level, leaves with parent -1, no items."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_domain_map.cc")
INC = os.path.join(ROOT, "training-operator_amd", "csrc")


def test_domain_map_matches_brute_force(tmp_path):
    exe = tmp_path / "test_domain_map"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wextra", "-Werror", "-I", INC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"(\d+) maps, (\d+) leaves, (\d+) items checked, 0 failures", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) >= 300 and int(m.group(2)) > 5000 and int(m.group(3)) > 5000
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
