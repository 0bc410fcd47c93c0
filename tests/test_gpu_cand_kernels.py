"""The kernels that write candidate lists from lists -- merge_shards_kernel, merge_ranked_kernel (system-scope and
plain loads), merge_kernel, empty_groups_kernel -- against a sorted union (cand_lists.py has the contract, the cases
and the reference).  Each test function runs its cases in one process of the driver built next to the library
(tests/cpp/cand_driver.cc) and judges the raw output buffers: n, flags, limit and every key exact, nothing written
past a list's n keys or behind the output."""
import os
import subprocess

import pytest

import cand_lists as cl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "training-operator_amd", "cand_driver")


def run(cases, tmp_path):
    """-> {case id: what is wrong}, after printing what was checked."""
    assert os.path.exists(DRIVER), "the driver is missing: build() makes it next to libplacement.so"
    for c in cases:
        cl.check_preconditions(c)
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cl.write_cases(src, cases)
    r = subprocess.run([DRIVER, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    wrong = {}
    for c, res in zip(cases, cl.read_outputs(dst, cases)):
        bad = cl.check_output(c, res)
        if bad:
            wrong[c.id] = bad[:4]
    groups = sum(c.Wg for c in cases)
    print("%d launches, %d lists checked, %d launches wrong" % (len(cases), groups, len(wrong)))
    return wrong


def test_selection_regimes(tmp_path):
    """topk_sort's one-level cut, two-level cut and bitonic fallback, through merge_shards and merge: shift 0, a key
    range past 2^63, the cut in bin 0 and bin 255, the (K+1)-th key the first of its bin, MG_SEL and MG_SEL + 1 keys
    in the cut at either level (test_cand_lists_cpu.py asserts that each case takes the branch it is named for)."""
    cases = cl.regime_cases()
    reached = {}
    for c in cases:
        name = cl.regime(cl.selected_keys(c, 0), c.K)[0]
        reached[(cl.KIND_NAMES[c.kind], name)] = reached.get((cl.KIND_NAMES[c.kind], name), 0) + 1
    print(sorted(reached.items()))
    assert all(reached.get((k, r), 0) >= 1 for k in ("merge_shards", "merge") for r in ("one", "two", "bitonic"))
    assert run(cases, tmp_path) == {}


def test_direct_sort_edges(tmp_path):
    """T of 0, 1, K, K + 1, K + 2, 2K + 2 and 2K + 3 keys at K of 1, 2, 63, 64, 65, 255 and 1023, dealt to 1, 2, 3 and
    16 ranks, through merge_shards and the rank merges."""
    cases = cl.grid_cases()
    direct = sum(1 for c in cases for want, _ in c.regimes.values() if want == "direct")
    print("direct-sort lists: %d, past the direct sort: %d" % (direct, sum(len(c.regimes) for c in cases) - direct))
    assert direct >= 100
    assert run(cases, tmp_path) == {}


def test_limits(tmp_path):
    assert run(cl.limit_cases(), tmp_path) == {}


def test_merge_ranked(tmp_path):
    assert run(cl.ranked_cases(), tmp_path) == {}


def test_refused_launches_write_nothing(tmp_path):
    assert run(cl.refused_cases(), tmp_path) == {}


def test_stride_gen_corrupt_and_xstatus(tmp_path):
    assert run(cl.every_kind_cases(), tmp_path) == {}


def test_merge_kernel(tmp_path):
    cases = cl.merge_cases()
    over = sum(1 for c in cases for g in range(c.Wg) if cl.reference(c, g).flags == 1)
    print("overflowed lists: %d" % over)
    assert over == 3
    assert run(cases, tmp_path) == {}


def test_empty_groups(tmp_path):
    assert run(cl.empty_cases(), tmp_path) == {}
