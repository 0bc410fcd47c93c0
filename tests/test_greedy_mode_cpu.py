"""CPU test of the greedy placement's mode decision (training-operator_amd/csrc/pe_greedy_mode.h: the
knobs, and which protocol a context and its knobs select): tests/cpp/test_greedy_mode.cc, built here with
plain g++ -- the header needs no HIP --, once as it is and once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_greedy_mode.cc")
INC = "-I" + os.path.join(ROOT, "training-operator_amd", "csrc")


def build_and_run(out, flags):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, INC, SRC, "-o", out], check=True,
                   timeout=300)
    p = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "\n0 failed checks" in p.stdout
    assert "FAIL" not in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    return p.stdout


def test_greedy_mode(tmp_path):
    out = build_and_run(str(tmp_path / "greedy_mode"), ["-O2"])
    for row in ("1 unsharded", "6 RCCL world 2", "7 RCCL world 17", "8 shared memory world 2, zero-copy",
                "9 shared memory world 2, PE_ZC_DEV_MERGE", "10 shared memory world 2, copying",
                "11 exchange callback world 2", "12 shared memory, small slots: no growth",
                "15 nothing set: the defaults"):
        assert "ok   " + row + "\n" in out, row


def test_greedy_mode_sanitized(tmp_path):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = subprocess.run(["g++", *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("no AddressSanitizer / UBSan runtime")
    build_and_run(str(tmp_path / "greedy_mode_san"), flags)
