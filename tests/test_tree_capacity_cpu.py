"""The hierarchy checker (tests/tree_capacity.py) against hand-worked cells, conservation between levels and
the C oracle's greedy placement; the selection rule over levels; the ABI surface of pe_gang_capacity_tree
that needs no GPU."""
import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
import oracle
import tree_capacity as TC
from placement import _abi, select_tree, synth
from test_go_binding import HIP_GO, go_calls, header_arity

# special_domains(): leaf 0 = node 2, leaf 2 = nodes 0 + 1, leaves 1 and 3 empty.  Leaves 0, 1 -> block 0;
# leaves 2, 3 -> block 1; block 0 -> the root, block 1 counts at its own level only.
SPECIAL_SIZES = [4, 2, 1]
SPECIAL_PARENT = [0, 0, 1, 1, 0, -1]


def test_special_cells_by_hand():
    cap, used, labels, island, D = DC.special_domains()
    assert D == SPECIAL_SIZES[0]
    res, lab = cap - used, synth.island_labels(labels, island)
    req = [c[0] for c in G.SPECIAL_CASES]
    need = [c[1] for c in G.SPECIAL_CASES]
    slots, nodes = TC.tables(res, lab, island, req, need, SPECIAL_SIZES, SPECIAL_PARENT)
    assert slots.shape == nodes.shape == (len(req), 7)
    for j, (leaf_slots, leaf_nodes) in enumerate(DC.special_tables()):
        for got, leaf in ((slots[j], leaf_slots), (nodes[j], leaf_nodes)):
            want = leaf + [leaf[0] + leaf[1], leaf[2] + leaf[3], leaf[0] + leaf[1]]
            assert [int(x) for x in got] == want, (j, req[j])
    C = G.CAP_MAX
    # all-zero request: node 2 (leaf 0) CAP_MAX, nodes 0 + 1 (leaf 2) 2 x CAP_MAX; the root holds block 0 only
    assert [int(x) for x in slots[0]] == [C, 0, 2 * C, 0, C, 2 * C, C] and [int(x) for x in nodes[0]] == [1, 0, 2, 0, 1, 2, 1]
    # [1, 1, 1, 1]: node 0 holds 4, node 1 saturates, node 2 has a zero dimension
    assert [int(x) for x in slots[3]] == [0, 0, 4 + C, 0, 0, 4 + C, 0] and [int(x) for x in nodes[3]] == [0, 0, 2, 0, 0, 2, 0]
    # [7, 0, 3, 9]: node 2 holds exactly one
    assert [int(x) for x in slots[4]] == [1, 0, 1 + C, 0, 1, 1 + C, 1]


@pytest.mark.parametrize("name", TC.TREES)
def test_conservation(name):
    """Each level's total is the lower level's total over the children that have a parent."""
    n = 700
    inv = synth.make_inventory(n, 7)
    island, sizes, parent = TC.tree(name, n)
    cap, used, lab, island = DC.with_islands(inv, island)
    req, need = synth.make_fit_jobs(40, 7)
    slots, nodes = TC.tables(cap - used, lab, island, req, need, sizes, parent)
    off = TC.offsets(sizes)
    assert slots.shape == (40, off[-1]) and slots[:, :off[1]].any()
    for t in (slots, nodes):
        for l in range(len(sizes) - 1):
            has = np.asarray(parent[off[l]:off[l + 1]]) >= 0
            np.testing.assert_array_equal(t[:, off[l + 1]:off[l + 2]].sum(axis=1), t[:, off[l]:off[l + 1]][:, has].sum(axis=1))
    if name in ("racks32", "four"):   # every leaf reaches the root: the root is the whole shard
        w_slots, _, w_nodes = G.capacity(cap - used, lab, req, (need | np.uint32(G.ISLAND)).astype(np.uint32))
        np.testing.assert_array_equal(slots[:, -1], w_slots)
        np.testing.assert_array_equal(nodes[:, -1], w_nodes)
    if name == "childless":
        assert not slots[:, off[1] + 1:off[2]:2].any() and not slots[:, off[2] + 1].any()
    if name == "fanin":
        start = np.bincount(np.asarray(parent[:off[1]]), minlength=sizes[1])
        assert sorted(start.tolist()) == sorted(TC.FANINS)


def placed(res, labels, count, req, need):
    _, st, _ = oracle.place_greedy(res, labels, *G.one_group_batch(count, req, need))
    return int(st[0]) == 0


@pytest.mark.parametrize("req,need", G.greedy_shapes())
def test_oracle_greedy_fills_an_upper_domain_exactly(req, need):
    """On the nodes of one upper-level domain alone the oracle's greedy places a one-group gang of exactly
    tree_slots pods and fails at tree_slots + 1."""
    inv = G.greedy_inventory()
    island = (np.arange(200) % 8).astype(np.int32)
    cap, used, lab, island = DC.with_islands(inv, island)
    res = cap - used
    sizes, parent = [8, 3, 2], [0, 0, 0, 1, 1, 2, 2, -1, 0, 0, 1]
    slots, nodes = TC.tables(res, lab, island, [req], [need], sizes, parent)
    leaf_parent = np.array(parent[:8])
    members = [(8 + p, np.isin(island, np.nonzero(leaf_parent == p)[0])) for p in range(3)]
    blocks_of = {0: [0, 1], 1: [2]}
    members += [(11 + z, np.isin(island, np.nonzero(np.isin(leaf_parent, blocks_of[z]))[0])) for z in range(2)]
    assert int(slots[0, 11]) >= 4 and sum(int(on.sum()) for _, on in members[:3]) == 175   # leaf 7 has no parent
    for col, on in members:
        s = int(slots[0, col])
        assert int(nodes[0, col]) <= int(on.sum())
        r, l = np.ascontiguousarray(res[:, on]), np.ascontiguousarray(lab[on])
        if s >= 1:
            assert placed(r, l, s, req, need), (col, s)
        assert not placed(r, l, s + 1, req, need), (col, s)


def test_selection_rule():
    sizes = [4, 2, 1]
    #                 racks          blocks   root
    table = np.array([[5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [5, 9, 5, 0, 14, 5, 19],
                      [6, 6, 6, 6, 12, 12, 24],
                      [6, 6, 6, 6, 12, 12, 24],
                      [0, 0, 0, 0, 0, 0, 0],
                      [2**54, 7, 2**54, 7, 2**54 + 7, 2**54 + 7, 2**55 + 14]], dtype=np.int64)
    count = np.array([5, 10, 15, 20, 10, 15, 5, 7, 13, 1, 2**31 - 1], dtype=np.int32)
    max_level = np.array([2, 2, 2, 2, 0, 1, 0, 2, 1, 2, 2], dtype=np.int32)
    level, dom, slots, feas = TC.select(table, count, sizes, max_level)
    # the lowest level wins (row 0: three racks hold 5, the smallest id of the smallest); only a block (1);
    # only the root (2); nowhere (3); max_level cuts (4: a block would hold it; 5: the root would);
    # best fit and a tie at an upper level (7: both blocks hold 12); required block, only the root holds it (8)
    assert level.tolist() == [0, 1, 2, -1, -1, -1, 0, 1, -1, -1, 0]
    assert dom.tolist() == [0, 0, 0, -1, -1, -1, 0, 0, -1, -1, 0]
    assert slots.tolist() == [5, 14, 19, 0, 0, 0, 5, 12, 0, 0, 2**54]
    assert feas.tolist() == [[3, 2, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0], [0, 1, 1], [0, 0, 1], [3, 2, 1], [0, 2, 1],
                             [0, 0, 1], [0, 0, 0], [2, 2, 1]]
    assert TC.select_row([3, 3, 6], 3, [2, 1]) == (0, 0, 3, [2, 1]) and TC.select_row([3, 3, 6], 4, [2, 1], 0) == (-1, -1, 0, [0, 1])
    assert TC.select_row([3, 5, 4, 12], 4, [3, 1]) == (0, 2, 4, [2, 1])          # best fit, not the first fit
    # max_level None = the top level
    for got, want in zip(TC.select(table, count, sizes), TC.select(table, count, sizes, np.full(11, 2))):
        np.testing.assert_array_equal(got, want)
    # the package's host helper (tables added over shards) follows the same rule
    for ml in (max_level, None):
        for got, want in zip(select_tree(table, count, sizes, ml), TC.select(table, count, sizes, ml)):
            assert got.dtype == want.dtype and got.shape == want.shape
            np.testing.assert_array_equal(got, want)
    rng = np.random.default_rng(3)
    sizes = [9, 4, 2, 1]
    t = rng.integers(0, 6, (300, 16)).astype(np.int64)
    c = rng.integers(1, 7, 300).astype(np.int32)
    ml = rng.integers(0, 4, 300).astype(np.int32)
    for got, want in zip(select_tree(t, c, sizes, ml), TC.select(t, c, sizes, ml)):
        np.testing.assert_array_equal(got, want)
    # one level: the rule of pe_gang_capacity_domains
    level, dom, slots, feas = select_tree(t[:, :9], c, [9])
    w_dom, w_slots, w_feas = DC.select(t[:, :9], c)
    np.testing.assert_array_equal(dom, w_dom)
    np.testing.assert_array_equal(slots, w_slots)
    np.testing.assert_array_equal(feas[:, 0], w_feas)
    np.testing.assert_array_equal(level, np.where(w_dom >= 0, 0, -1))
    with pytest.raises(ValueError):
        select_tree(t, np.zeros(300, dtype=np.int32), sizes)
    with pytest.raises(ValueError):
        select_tree(t, c, sizes, np.full(300, 4))
    with pytest.raises(ValueError):
        select_tree(t, c, [9, 4, 2])


def test_bindings():
    """The header declares pe_gang_capacity_tree with 15 arguments; _abi.py and hip.go bind it so."""
    assert header_arity()["pe_gang_capacity_tree"] == 15
    res, args = _abi.SIGNATURES["pe_gang_capacity_tree"]
    assert len(args) == 15 and args[1] is _abi.i64 and args[6] is _abi.i32
    assert go_calls(HIP_GO)["pe_gang_capacity_tree"] == {15}
    assert "func (e *Engine) GangCapacityTree(" in open(HIP_GO).read()
    assert _abi.PE_MAX_LEVELS == 4
    header = open(_abi.HEADER).read()
    assert "#define PE_MAX_LEVELS 4" in header and "#define PE_ABI_VERSION 7" in header
    lib = _abi.load()
    assert lib.pe_gang_capacity_tree(None, 0, None, None, None, None, 1, None, None, None, None, None, None, None,
                                     None) == _abi.PE_EINVAL
