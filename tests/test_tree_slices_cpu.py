"""The slice checker (tests/tree_slices.py) on the CPU: its two statements of pe_gang_slice_tree's rule against each
other, the consequences the header promises job by job, the z = 1 identity with tree_split, the hand-made traps,
the C oracle's placement of every node-level part as island groups, and the ABI surface that needs no GPU."""
import numpy as np
import pytest

import domain_placement as DP
import tree_capacity as TC
import tree_slices as SL
import tree_split as TS
from placement import _abi
from test_go_binding import HIP_GO, go_calls, header_arity

NAMED = [(name, n) for n in (257, 1025) for name in TC.TREES]


def differs(a, b):
    return any(not np.array_equal(getattr(a, f), getattr(b, f)) for f in TS.FIELDS)


@pytest.mark.parametrize("name,n", NAMED)
def test_statements_agree_on_named_trees(name, n):
    cases = SL.named_cases(name, n)
    L = len(TC.tree(name, n)[1])
    assert set(cases) == {(z, sl) for z in SL.SIZES for sl in range(SL.NODE, L)}
    for (z, sl), (case, probe) in cases.items():
        what = f"z {z} sl {sl}"
        want = case.want(TS.walk)
        SL.same(case.want(TS.threshold), want, what + " threshold")
        SL.same(case.want(TS.threshold, SL.MAX_PARTS), case.want(TS.walk, SL.MAX_PARTS), what + " threshold, all parts")
        for j, r in enumerate(case.want_rows()):
            SL.consequences(case.rows[j], case.table[j], int(case.count[j]), z, sl, case.sizes, case.parent, r)
        # what every case must show, on the checker alone
        parts = want.parts
        split = case.split_want()
        if L == 1:
            assert set(parts.tolist()) == {0, 1} and (want.spread == (parts == 1)[:, None]).all(), what
            assert (z == 1) != differs(want, split), what
            continue
        assert (parts > 1).any() and (parts == 1).any() and (parts == 0).any() and (parts == SL.TOO_MANY).any(), what
        p, lvl = parts[probe], want.level[probe]
        assert p[0] >= 1 and lvl[0] == max(sl, 0)                   # one slice: the slice level itself
        assert lvl[1] > max(sl, 0) or lvl[1] == -1                  # one more than the largest level-m domain
        assert lvl[2] >= 0 and p[3] == 0 and lvl[3] == -1           # the top domain, and one more than it
        assert p[4] == case.max_parts >= 2 and p[5] == SL.TOO_MANY
        assert case.want(TS.walk, SL.MAX_PARTS).parts[probe][5] == case.max_parts + 1
        if z == 1 and sl <= 0:
            # the identity: every shared output bit-equal to tree_split.split's, units the selected domain's slots
            SL.same(want, split, what + " identity", TS.FIELDS)
            sel = TC.select(case.table, case.count, case.sizes, case.max_level)
            np.testing.assert_array_equal(want.units, sel[2])
        else:
            assert differs(want, split), what


@pytest.mark.parametrize("trap", SL.TRAPS, ids=[t[0] for t in SL.TRAPS])
def test_traps(trap):
    name, _, _, sizes, _, count, z, sl, level, domain, units, parts, spread = trap
    case = SL.trap_case(trap)
    for step in (TS.walk, TS.threshold):
        want = case.want(step)
        assert want.lists[0] == parts, (name, step.__name__)
        assert (want.level[0], want.domain[0], want.units[0]) == (level, domain, units)
        assert want.spread[0].tolist() == spread and want.parts[0] == len(parts)
    r = case.want_rows()[0]
    SL.consequences(case.rows[0], case.table[0], count, z, sl, case.sizes, case.parent, r)
    split = case.split_want()
    if name == "block_of_two_racks":     # counting pods says yes and cuts a slice in half
        assert split.lists[0] == [(0, 12), (1, 12)]
    if name == "two_nodes_node_level":   # floor(slots / z) = 3 would say yes
        assert case.table[0][0] // z == 3 and case.rows[0][0] == 2
    if name == "units_tie":              # best fit by slots
        assert split.lists[0] == [(1, 8)]
    if name == "best_fit_last_in_units":
        assert [(d, n // z) for d, n in parts] == TS.TRAPS[0][5]


@pytest.mark.parametrize("name", [t for t in TC.TREES])
def test_oracle_places_node_level_parts(name):
    """sl = NODE: part (leaf, a * z) as ONE job of a island groups of z pods in its leaf; the parts of one answer in
    one batch.  The C oracle (domain_placement.place) places every job."""
    cases = SL.named_cases(name, 257)
    done = 0
    for z in (2, 3, 8):
        case, _ = cases[(z, SL.NODE)]
        want = case.want()
        res = case.cap - case.used
        lab = np.where(case.island >= 0, case.labels | np.uint32(DP.ISLAND), case.labels).astype(np.uint32)
        for j in np.flatnonzero(want.parts >= 1)[:12]:
            need = int(case.need[j]) | DP.ISLAND
            jobs = [(leaf, 0, [(z, case.req[j].tolist(), need)] * (pods // z)) for leaf, pods in want.lists[j]]
            batch, dom = DP.make_batch(jobs)
            _, status, _ = DP.place(res, lab, case.island, batch, dom, 0, case.sizes, case.parent)
            assert not np.asarray(status).any(), (z, j, want.lists[j])
            done += len(jobs)
    assert done > 20


def test_bindings():
    """The header declares pe_gang_slice_tree with 19 arguments; _abi.py and hip.go bind it so."""
    assert header_arity()["pe_gang_slice_tree"] == 19
    res, args = _abi.SIGNATURES["pe_gang_slice_tree"]
    assert len(args) == 19 and args[1] is _abi.i64 and args[8] is _abi.i32 and args[11] is _abi.i32
    assert go_calls(HIP_GO)["pe_gang_slice_tree"] == {19}
    assert "func (e *Engine) GangSliceTree(" in open(HIP_GO).read()
    assert _abi.PE_SLICE_NODE == -1 == SL.NODE
    header = open(_abi.HEADER).read()
    assert "#define PE_SLICE_NODE (-1)" in header and "#define PE_ABI_VERSION 7" in header
    lib = _abi.load()
    assert lib.pe_gang_slice_tree(None, 0, None, None, None, None, None, None, 1, None, None, 1, None, None, None, None,
                                  None, None, None) == _abi.PE_EINVAL
