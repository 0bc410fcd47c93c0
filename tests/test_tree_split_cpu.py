"""The split checker (tests/tree_split.py) on the CPU: its two statements of pe_gang_split_tree's rule against each
other, the consequences the header promises job by job, the hand-made traps, the C oracle's greedy placement of
every part, the package's host helper, and the ABI surface that needs no GPU."""
import numpy as np
import pytest

import gang_capacity as G
import oracle
import tree_capacity as TC
import tree_split as TS
from placement import _abi, split_tree
from test_go_binding import HIP_GO, go_calls, header_arity

NAMED = [(name, n) for n in (257, 1025) for name in TC.TREES]
FANS = [(f, kind) for f in (1, 2, 63, 64, 65, 200) for kind in TS.FAN_KINDS]


def jobs_hold(case, want):
    kids = TS.children(case.sizes, case.parent)
    for j in range(len(case.count)):
        ml = None if case.max_level is None else int(case.max_level[j])
        r = TS.split_row(case.table[j], int(case.count[j]), case.sizes, kids, ml, case.max_parts)
        assert r[2] == want.parts[j]
        TS.consequences(case.table[j], int(case.count[j]), case.sizes, case.parent, kids, r)


@pytest.mark.parametrize("name,n", NAMED)
def test_statements_agree_on_named_trees(name, n):
    case = TS.named_case(name, n)
    want = case.want(TS.walk)
    TS.same(case.want(TS.threshold), want, "threshold")
    TS.same(case.want(TS.threshold, TS.MAX_PARTS), case.want(TS.walk, TS.MAX_PARTS), "threshold, all parts")
    jobs_hold(case, want)
    for mp in (case.max_parts, TS.MAX_PARTS):
        TS.same(TS.split_wide(case.table, np.arange(len(case.count)), case.count, case.sizes, case.parent, case.max_level, mp),
                case.want(max_parts=mp),
                "split_wide")
    # what every case must show, on the checker alone
    parts = want.parts
    assert (parts == 1).any() and (parts == 0).any()
    if len(case.sizes) > 1:
        assert (parts > 1).any() and (parts == TS.TOO_MANY).any()
        p = parts[case.probe]
        lvl = want.level[case.probe]
        # the six derived counts of the probe shape, in order: 1, a leaf and one more, the top domain, one more than
        # it, exactly max_parts parts, max_parts + 1 parts
        assert p[0] == 1 and lvl[0] == 0
        assert lvl[1] >= 1 and (p[1] >= 2 or p[1] == TS.TOO_MANY)
        assert lvl[2] == want.level[case.probe].max() >= 1
        assert p[3] == 0 and lvl[3] == -1
        assert p[4] == case.max_parts >= 2 and p[5] == TS.TOO_MANY
        all_parts = case.want(TS.walk, TS.MAX_PARTS).parts[case.probe]
        assert all_parts[5] == case.max_parts + 1 and all_parts[2] >= all_parts[5]
        # a required level below the one that holds the gang leaves nothing to split
        cut = parts[len(parts) - 2 * len(p):len(parts) - len(p)]   # the probe shape at max_level 0
        assert cut[0] == 1 and (cut[1:] == 0).all()
    else:
        assert set(parts.tolist()) == {0, 1} and (want.spread == (parts == 1)[:, None]).all()


@pytest.mark.parametrize("f,kind", FANS)
def test_statements_agree_on_fan_trees(f, kind):
    case = TS.fan_case(f, kind)
    want = case.want(TS.walk)
    TS.same(case.want(TS.threshold), want, "threshold")
    TS.same(case.want(TS.threshold, TS.MAX_PARTS), case.want(TS.walk, TS.MAX_PARTS), "threshold, all parts")
    jobs_hold(case, want)
    if f >= 3:
        assert (want.parts == case.max_parts).any() and (want.parts == TS.TOO_MANY).any() and (want.parts == 0).any()
    # a child without slots is never a part
    for j, lst in enumerate(want.lists):
        assert all(case.table[j][leaf] >= n >= 1 for leaf, n in lst)


def test_random_child_lists():
    """The two steps on child lists with ties and zeros, every allotment of each."""
    rng = np.random.default_rng(4)
    for _ in range(400):
        n = int(rng.integers(1, 10))
        slots = [int(x) for x in rng.choice([0, 0, 1, 2, 3, 5, 5, 8, 13], n)]
        ids = sorted(int(x) for x in rng.choice(50, n, replace=False))
        for a in range(1, sum(slots) + 1):
            w = TS.walk(ids, slots, a)
            assert w == TS.threshold(ids, slots, a), (ids, slots, a)
            assert sum(p for _, p in w) == a and len({c for c, _ in w}) == len(w)
            k = 1
            while sum(sorted(slots, reverse=True)[:k]) < a:
                k += 1
            assert len(w) == k


@pytest.mark.parametrize("trap", TS.TRAPS, ids=[t[0] for t in TS.TRAPS])
def test_traps(trap):
    name, leaf, sizes, parent, count, parts, spread = trap
    case = TS.trap_case(trap)
    np.testing.assert_array_equal(case.table, TS.trap_tables(trap))      # one GPU per pod: a leaf's slots are its GPUs
    for step in (TS.walk, TS.threshold):
        want = case.want(step)
        assert want.lists[0] == parts, (name, step.__name__)
        assert want.spread[0].tolist() == spread and want.parts[0] == len(parts)
        assert want.level[0] == len(sizes) - 1 and want.domain[0] == 0
    jobs_hold(case, case.want())
    if name == "best_fit_last":   # what plain descending order would have answered
        assert parts != [(0, 10), (1, 3)]


def test_traps_cut_by_max_parts():
    case = TS.trap_case(TS.TRAPS[1])   # three parts
    for mp, parts in ((1, TS.TOO_MANY), (2, TS.TOO_MANY), (3, 3), (4, 3)):
        want = case.want(max_parts=mp)
        assert want.parts[0] == parts and want.level[0] == 1 and want.domain[0] == 0
        assert want.part_domain.shape == (1, mp)
        if parts < 0:
            assert (want.part_domain == -1).all() and not want.part_pods.any() and not want.spread.any()


@pytest.mark.parametrize("name", [t for t in TC.TREES if t != "flat"])
def test_oracle_places_every_part(name):
    """Each part of a job as a one-group gang on the nodes of its leaf alone: the C oracle's greedy places it.
    The leaves of a job are distinct, so its parts never share a node."""
    case = TS.named_case(name, 257)
    res = case.cap - case.used
    lab = np.where(case.island >= 0, case.labels | np.uint32(1 << 31), case.labels).astype(np.uint32)
    want = case.want()
    done = 0
    for j in np.flatnonzero(want.parts >= 1):
        req, need = case.req[j], case.need[j]
        for leaf, pods in want.lists[j]:
            on = case.island == leaf
            _, st, _ = oracle.place_greedy(np.ascontiguousarray(res[:, on]), np.ascontiguousarray(lab[on]),
                                           *G.one_group_batch(pods, req, need))
            assert int(st[0]) == 0, (j, leaf, pods)
            done += 1
    assert done > 20


@pytest.mark.parametrize("name,n", [("racks32", 257), ("four", 1025), ("orphans", 257), ("permuted", 257), ("flat", 257)])
def test_split_tree_helper(name, n):
    """placement.split_tree, the host form for tables added over shards, against the checker."""
    case = TS.named_case(name, n)
    for mp in (case.max_parts, TS.MAX_PARTS):
        got = split_tree(case.table, case.count, case.sizes, case.parent, case.max_level, mp)
        TS.same(got, case.want(max_parts=mp), f"max_parts {mp}")
    got = split_tree(case.table, case.count, case.sizes, case.parent)    # max_level None, every part
    TS.same(got, TS.split(case.table, case.count, case.sizes, case.parent), "defaults")
    for t in TS.TRAPS:
        c = TS.trap_case(t)
        TS.same(split_tree(c.table, c.count, c.sizes, c.parent, None, 8), c.want(), t[0])
    with pytest.raises(ValueError):
        split_tree(case.table, case.count, case.sizes, case.parent, None, 0)
    with pytest.raises(ValueError):
        split_tree(case.table, case.count, case.sizes, case.parent, None, TS.MAX_PARTS + 1)
    with pytest.raises(ValueError):
        split_tree(case.table, np.zeros_like(case.count), case.sizes, case.parent)
    if len(case.sizes) > 1:
        with pytest.raises(ValueError):
            split_tree(case.table, case.count, case.sizes, case.parent[:-1])


def test_bindings():
    """The header declares pe_gang_split_tree with 16 arguments; _abi.py and hip.go bind it so."""
    assert header_arity()["pe_gang_split_tree"] == 16
    res, args = _abi.SIGNATURES["pe_gang_split_tree"]
    assert len(args) == 16 and args[1] is _abi.i64 and args[6] is _abi.i32 and args[9] is _abi.i32
    assert go_calls(HIP_GO)["pe_gang_split_tree"] == {16}
    assert "func (e *Engine) GangSplitTree(" in open(HIP_GO).read()
    assert _abi.PE_MAX_SPLIT_PARTS == 1024 == TS.MAX_PARTS and _abi.PE_SPLIT_TOO_MANY == -1 == TS.TOO_MANY
    header = open(_abi.HEADER).read()
    assert "#define PE_MAX_SPLIT_PARTS 1024" in header and "#define PE_SPLIT_TOO_MANY (-1)" in header
    assert "#define PE_ABI_VERSION 7" in header
    lib = _abi.load()
    assert lib.pe_gang_split_tree(None, 0, None, None, None, None, 1, None, None, 1, None, None, None, None, None,
                                  None) == _abi.PE_EINVAL
