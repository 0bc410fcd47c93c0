"""pe_gang_capacity_tree on the GPU against the Python-integer checker (tests/tree_capacity.py): every cell
of both tables and every selection output of every job compared, nothing sampled."""
import itertools

import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
import tree_capacity as TC
from placement import Engine, PlacementError, _abi, select_tree, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)
COUNTS = np.array([1, 8, 40, 200, 1000, 5000, 30000, 2**31 - 1], dtype=np.int32)


def counts_for(J):
    return np.resize(COUNTS, J).astype(np.int32)


def levels_for(J, n_levels):
    """A max_level per job that meets every count of counts_for with every level."""
    return ((np.arange(J) // len(COUNTS) + np.arange(J)) % n_levels).astype(np.int32)


def same_tables(got, want_slots, want_nodes):
    assert got.tree_slots.dtype == np.int64 and got.tree_nodes.dtype == np.int64
    np.testing.assert_array_equal(got.tree_slots, want_slots, err_msg="tree_slots")
    np.testing.assert_array_equal(got.tree_nodes, want_nodes, err_msg="tree_nodes")


def same_selection(got, want_slots, count, sizes, max_level):
    level, dom, slots, feas = TC.select(want_slots, count, sizes, max_level)
    assert got.level.dtype == np.int32 and got.domain.dtype == np.int32 and got.domain_slots.dtype == np.int64
    assert got.feasible.dtype == np.int32 and got.feasible.shape == (len(count), len(sizes))
    np.testing.assert_array_equal(got.level, level, err_msg="level")
    np.testing.assert_array_equal(got.domain, dom, err_msg="domain")
    np.testing.assert_array_equal(got.domain_slots, slots, err_msg="domain_slots")
    np.testing.assert_array_equal(got.feasible, feas, err_msg="feasible")


def check(e, m, island, sizes, parent, req, need, count, max_level="cycle"):
    """The engine's answers (tables + selection, the selection alone, the preferred-lowest form) against the
    cap matrix m."""
    if isinstance(max_level, str):
        max_level = levels_for(len(count), len(sizes))
    want_slots, want_nodes = TC.tables_of(m, island, sizes, parent)
    got = e.gang_capacity_tree(req, need, count, max_level, sizes, parent)
    same_tables(got, want_slots, want_nodes)
    same_selection(got, want_slots, count, sizes, max_level)
    lean = e.gang_capacity_tree(req, need, count, max_level, sizes, parent, tables=False)
    assert lean.tree_slots is None and lean.tree_nodes is None
    same_selection(lean, want_slots, count, sizes, max_level)
    if max_level is not None:
        same_selection(e.gang_capacity_tree(req, need, count, None, sizes, parent, tables=False), want_slots, count, sizes,
                       None)
    return want_slots, want_nodes


_sized = {}


def sized(n):
    """Per shard size: the inventory, 24 job shapes and their cap matrix (no need carries the island bit, so
    the matrix is the same under every hierarchy)."""
    if n not in _sized:
        inv = synth.make_inventory(n, 7)
        req, need = synth.make_fit_jobs(24, 7 + n)
        assert not (need & ISLAND).any()
        _sized[n] = (inv, req, need, G.capacity_matrix(inv.residual(), inv.labels, req, need))
    return _sized[n]


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n_nodes", [1, 1023, 1024, 1025, 2500])
def test_sizes_and_trees(n_nodes, name):
    inv, req, need, m = sized(n_nodes)
    island, sizes, parent = TC.tree(name, n_nodes)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    if name == "permuted":   # removed slots too: they count nowhere at any level
        gone = np.arange(n_nodes)[3::11]
        if len(gone):
            e.update_nodes(gone, np.full(len(gone), _abi.PE_NODE_REMOVE, dtype=np.uint8))
        island = island.copy()
        island[gone] = -1
    want_slots, want_nodes = check(e, m, island, sizes, parent, req, need, counts_for(24))
    if name in ("racks32", "four"):
        # every leaf reaches the root: the root is pe_gang_capacity's answer for need | ISLAND
        slots, _, nodes = e.gang_capacity(req, (need | ISLAND).astype(np.uint32))
        got = e.gang_capacity_tree(req, need, None, None, sizes, parent)
        np.testing.assert_array_equal(got.tree_slots[:, -1], slots)
        np.testing.assert_array_equal(got.tree_nodes[:, -1], nodes)
        assert got.level is None and got.domain is None and slots.any()
    if n_nodes >= 1023:
        assert want_slots[:, sizes[0]:].any() == (len(sizes) > 1)
    e.close()


@pytest.mark.parametrize("layout", DC.LAYOUTS)
def test_one_level_is_gang_capacity_domains(layout):
    n = 2500
    inv, req, need, m = sized(n)
    island, D = DC.layout(layout, n)
    count = counts_for(24)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    dom = e.gang_capacity_domains(req, need, count, D)
    for parent in (None, np.zeros(0, dtype=np.int32)):
        got = e.gang_capacity_tree(req, need, count, None, [D], parent)
        np.testing.assert_array_equal(got.tree_slots, dom.dom_slots)
        np.testing.assert_array_equal(got.tree_nodes, dom.dom_nodes)
        np.testing.assert_array_equal(got.domain, dom.domain)
        np.testing.assert_array_equal(got.domain_slots, dom.domain_slots)
        np.testing.assert_array_equal(got.feasible, dom.feasible[:, None])
        np.testing.assert_array_equal(got.level, np.where(dom.domain >= 0, 0, -1))
    lean = e.gang_capacity_tree(req, need, count, np.zeros(24, dtype=np.int32), [D], None, tables=False)
    np.testing.assert_array_equal(lean.domain, dom.domain)
    np.testing.assert_array_equal(lean.domain_slots, dom.domain_slots)
    check(e, m, island, [D], None, req, need, count)
    e.close()


@pytest.mark.parametrize("fan_in", [1, 2, 3, 31, 32, 33, 63, 64, 65, 200])
def test_width_boundaries(fan_in):
    """The lanes per parent follow the level's largest fan-in: one level per width and its neighbours."""
    n = 1025
    inv, req, need, m = sized(n)
    sizes, parent = TC.fan_tree(fan_in)
    island = (np.arange(n) % sizes[0]).astype(np.int32)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    want_slots, _ = check(e, m, island, sizes, parent, req, need, counts_for(24))
    np.testing.assert_array_equal(want_slots[:, -2], want_slots[:, 1:sizes[0]].sum(axis=1))
    assert want_slots[:, -2].any() and want_slots[:, -1].any()
    e.close()


def test_childless_levels():
    """A level whose parents all have no child, under a level that has some: zeros, never chosen."""
    n = 1025
    inv, req, need, m = sized(n)
    island = (np.arange(n) // 32).astype(np.int32)
    sizes = [33, 70, 5, 2]
    parent = np.concatenate([np.arange(33) % 3, np.full(70, -1), [0, 1, 0, -1, 1]]).astype(np.int32)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    want_slots, want_nodes = check(e, m, island, sizes, parent, req, need, counts_for(24))
    assert want_slots[:, 33:36].any() and not want_slots[:, 36:].any() and not want_nodes[:, 36:].any()
    got = e.gang_capacity_tree(req, need, counts_for(24), None, sizes, parent, tables=False)
    assert not got.feasible[:, 2:].any() and (got.level <= 1).all()
    e.close()


def test_selection():
    """64 equal nodes in racks of 8, blocks of 4 racks, one root; rack 3 loses one node, rack 6 two."""
    GiB = G.GiB
    cap = np.tile(np.array([[8000], [64 * GiB], [8], [100 * GiB]], dtype=np.int64), (1, 64))
    island = (np.arange(64) // 8).astype(np.int32)
    sizes, parent = [8, 2, 1], np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 0], dtype=np.int32)
    e = Engine(0)
    e.load_nodes(cap, np.zeros_like(cap), np.zeros(64, dtype=np.uint32), island)
    e.update_nodes([24, 48, 49], [_abi.PE_NODE_REMOVE] * 3)
    island[[24, 48, 49]] = -1
    small, big = [1000, 8 * GiB, 1, 0], [8000, 8 * GiB, 8, 100 * GiB]     # 8 per node / 1 per node
    # a gang that fits a rack, only a block, only the root, nowhere; equal shapes with different counts,
    # recurring out of order, in one batch
    jobs = [(small, 48), (small, 49), (small, 65), (small, 241), (small, 249), (small, 489), (big, 7), (big, 9), (big, 31),
            (big, 62), (small, 65), (small, 48), (big, 9), (small, 240), (small, 248), (small, 488)]
    req = np.array([j[0] for j in jobs], dtype=np.int64)
    count = np.array([j[1] for j in jobs], dtype=np.int32)
    J = len(jobs)
    got = e.gang_capacity_tree(req, None, count, None, sizes, parent)
    assert got.tree_slots[0].tolist() == [64, 64, 64, 56, 64, 64, 48, 64, 248, 240, 488]
    assert got.tree_nodes[6].tolist() == [8, 8, 8, 7, 8, 8, 6, 8, 31, 30, 61] == got.tree_slots[6].tolist()
    assert got.level.tolist() == [0, 0, 1, 1, 2, -1, 0, 1, 1, -1, 1, 0, 1, 1, 1, 2]
    assert got.domain.tolist() == [6, 3, 1, 0, 0, -1, 3, 1, 0, -1, 1, 6, 1, 1, 0, 0]
    assert got.domain_slots.tolist() == [48, 56, 240, 248, 488, 0, 7, 30, 31, 0, 240, 48, 30, 240, 248, 488]
    assert got.feasible.tolist() == [[8, 2, 1], [7, 2, 1], [0, 2, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0], [7, 2, 1], [0, 2, 1],
                                     [0, 1, 1], [0, 0, 0], [0, 2, 1], [8, 2, 1], [0, 2, 1], [0, 2, 1], [0, 1, 1], [0, 0, 1]]
    # required at rack / at block level: what only a higher level holds is refused, the counts stay
    for r in (0, 1):
        cut = e.gang_capacity_tree(req, None, count, np.full(J, r, dtype=np.int32), sizes, parent, tables=False)
        ok = (got.level >= 0) & (got.level <= r)
        np.testing.assert_array_equal(cut.level, np.where(ok, got.level, -1))
        np.testing.assert_array_equal(cut.domain, np.where(ok, got.domain, -1))
        np.testing.assert_array_equal(cut.domain_slots, np.where(ok, got.domain_slots, 0))
        np.testing.assert_array_equal(cut.feasible, got.feasible)
        assert (cut.level != got.level).any()
    # equal shapes and counts with different max_level in one batch: three picks per (shape, count)
    req3, count3 = np.repeat(req, 3, axis=0), np.repeat(count, 3)
    ml3 = np.tile(np.array([2, 0, 1], dtype=np.int32), J)
    m = G.capacity_matrix(e.read_residuals(), np.where(island >= 0, ISLAND, 0).astype(np.uint32), req3, None)
    check(e, m, island, sizes, parent, req3, None, count3, ml3)
    mixed = e.gang_capacity_tree(req3, None, count3, ml3, sizes, parent, tables=False)
    np.testing.assert_array_equal(mixed.level[0::3], got.level)
    np.testing.assert_array_equal(mixed.level[1::3], np.where(got.level == 0, 0, -1))
    e.close()


def test_table_chunks():
    """level_size = [65536, 512, 1]: the device holds the tables of 84 shapes at a time, the batch has 200."""
    n, sizes = 1025, [65536, 512, 1]
    assert (64 << 20) // (12 * sum(sizes)) == 84
    inv = synth.make_inventory(n, 7)
    ids = (np.arange(n) * 63).astype(np.int32)           # ascending, up to 64512
    parent = np.concatenate([np.arange(65536) // 128, np.zeros(512)]).astype(np.int32)
    J = 200
    req = np.array([[100 * (j + 1), G.GiB, 0, 0] for j in range(J)], dtype=np.int64)
    count = np.resize(np.array([1, 40, 300, 2000, 10**6], dtype=np.int32), J)
    max_level = (np.arange(J) % 3).astype(np.int32)
    c_slots, c_nodes = DC.tables_of(G.capacity_matrix(inv.residual(), inv.labels, req, None), np.arange(n), n)
    want = []
    for c in (c_slots, c_nodes):    # small integers: int64 sums are exact
        leaf = np.zeros((J, 65536), dtype=np.int64)
        leaf[:, ids] = c
        block = leaf.reshape(J, 512, 128).sum(axis=2)
        want.append(np.concatenate([leaf, block, block.sum(axis=1, keepdims=True)], axis=1))
    # the checker's roll-up on a few rows (66049 columns each)
    rows = [0, 83, 84, 199]
    np.testing.assert_array_equal(TC.rollup(want[0][rows, :65536], sizes, parent), want[0][rows])
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, ids)
    got = e.gang_capacity_tree(req, None, count, max_level, sizes, parent)
    np.testing.assert_array_equal(got.tree_slots, want[0])
    np.testing.assert_array_equal(got.tree_nodes, want[1])
    sel = select_tree(want[0], count, sizes, max_level)
    for r in rows:
        assert TC.select_row(want[0][r], int(count[r]), sizes, int(max_level[r])) == \
            (int(sel[0][r]), int(sel[1][r]), int(sel[2][r]), sel[3][r].tolist())
    assert len(set(sel[0].tolist())) == 4                 # every level and none
    lean = e.gang_capacity_tree(req, None, count, max_level, sizes, parent, tables=False)
    for a, b, c in zip(got[2:], lean[2:], sel):
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, c)
    e.close()


def test_state_changes():
    n = 2500
    inv, req, need, m0 = sized(n)
    count = counts_for(24)
    island, sizes, parent = TC.tree("racks32", n)
    island = island.copy()
    labels = inv.labels.copy()
    D = sizes[0]
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, labels, island)
    before, _ = check(e, m0, island, sizes, parent, req, need, count)

    def now():
        return G.capacity_matrix(e.read_residuals(), synth.island_labels(labels, island), req, need)

    # placements lower the residuals
    _, st = e.place_batch(synth.make_jobs(100, 7, "mixed"))
    assert (st == 0).any()
    after, _ = check(e, now(), island, sizes, parent, req, need, count)
    assert (after[:, D:] < before[:, D:]).any()
    # a node moves to another leaf, in another block (the slot is rewritten: its residual is cap - used again)
    slot = int(np.argmax(np.asarray(m0 >= 1, dtype=bool).sum(axis=0)))
    old, new = int(island[slot]), (int(island[slot]) + 40) % D
    assert parent[old] != parent[new]
    e.update_nodes([slot], [_abi.PE_NODE_SET], inv.cap[:, slot][None], inv.used[:, slot][None], labels[slot:slot + 1], [new])
    island[slot] = new
    moved, _ = check(e, now(), island, sizes, parent, req, need, count)
    assert (moved[:, D + parent[new]] > after[:, D + parent[new]]).any()
    assert (moved[:, D + parent[old]] <= after[:, D + parent[old]]).all()
    # a node is removed
    e.update_nodes([slot], [_abi.PE_NODE_REMOVE])
    island[slot], labels[slot] = -1, 0
    removed, _ = check(e, now(), island, sizes, parent, req, need, count)
    assert (removed[:, -1] < moved[:, -1]).any()
    # a node is added: the free slot gets another node, in yet another leaf
    src, dom = (slot + 1) % n, (new + 7) % D
    e.update_nodes([slot], [_abi.PE_NODE_SET], inv.cap[:, src][None], inv.used[:, src][None], inv.labels[src:src + 1], [dom])
    island[slot], labels[slot] = dom, inv.labels[src]
    check(e, now(), island, sizes, parent, req, need, count)
    # residuals reset
    e.reset_residuals()
    check(e, now(), island, sizes, parent, req, need, count)
    # the same inventory under another hierarchy: the parent map is an argument, nothing of it is kept
    _, sizes4, parent4 = TC.tree("orphans", n)
    check(e, now(), island, sizes4, parent4, req, need, count)
    # a reload with other islands, another size
    inv2, req2, need2, m2 = sized(1025)
    island2, sizes2, parent2 = TC.tree("permuted", 1025)
    e.load_nodes(inv2.cap, inv2.used, inv2.labels, island2)
    check(e, m2, island2, sizes2, parent2, req2, need2, count)
    check(e, G.capacity_matrix(inv2.residual(), inv2.labels, req, need), island2, sizes2, parent2, req, need, count)
    e.close()


@pytest.mark.parametrize("n_nodes", [2500, 2])
def test_shards(n_nodes):
    """Three shard contexts (n_nodes = 2: the first is empty): their tables add up to the unsharded tables."""
    inv, req, need, m = sized(n_nodes)
    _, sizes, parent = TC.tree("four", n_nodes)
    island = (np.arange(n_nodes) % sizes[0]).astype(np.int32)        # every leaf spans the shards
    count = counts_for(24)
    max_level = levels_for(24, len(sizes))
    want_slots, want_nodes = TC.tables_of(m, island, sizes, parent)
    slots = np.zeros_like(want_slots)
    nodes = np.zeros_like(want_nodes)
    empty = 0
    for r in range(3):
        s = Engine(0, rank=r, world_size=3, exchange=lambda b: b * 3)
        s.load_nodes(inv.cap, inv.used, inv.labels, island)
        b, e = s.shard_range()
        got = s.gang_capacity_tree(req, need, None, None, sizes, parent)
        same_tables(got, *TC.tables_of(m[:, b:e], island[b:e], sizes, parent))
        if b == e:
            empty += 1
            assert not got.tree_slots.any() and not got.tree_nodes.any()
        slots += got.tree_slots
        nodes += got.tree_nodes
        for tables in (True, False):                     # one shard's table must not be selected from
            with pytest.raises(PlacementError) as ei:
                s.gang_capacity_tree(req, need, count, max_level, sizes, parent, tables=tables)
            assert ei.value.code == _abi.PE_EINVAL and "shard" in str(ei.value)
        s.close()
    np.testing.assert_array_equal(slots, want_slots)
    np.testing.assert_array_equal(nodes, want_nodes)
    assert empty == (1 if n_nodes == 2 else 0)
    one = Engine(0)
    one.load_nodes(inv.cap, inv.used, inv.labels, island)
    whole = one.gang_capacity_tree(req, need, count, max_level, sizes, parent)
    same_tables(whole, slots, nodes)
    for got, dev, want in zip(select_tree(slots, count, sizes, max_level), whole[2:],
                              TC.select(want_slots, count, sizes, max_level)):
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, dev)
    one.close()


def raw_call(e, req, need, count, max_level, sizes, parent, outs):
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    parent = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    return e.lib.pe_gang_capacity_tree(e.h, req.shape[0], req.ctypes.data, ptr(need), ptr(count), ptr(max_level), len(sizes),
                                       sizes.ctypes.data, ptr(parent), *[ptr(o) for o in outs])


def test_optional_outputs():
    inv, req, need, m = sized(1023)
    island, sizes, parent = TC.tree("racks32", 1023)
    count = counts_for(24)
    max_level = levels_for(24, 3)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    full = e.gang_capacity_tree(req, need, count, max_level, sizes, parent)
    same_tables(full, *TC.tables_of(m, island, sizes, parent))
    dtypes = (np.int64, np.int64, np.int32, np.int32, np.int64, np.int32)
    for on in itertools.product((False, True), repeat=6):
        outs = [np.full(full[k].shape, -7, dtype=dtypes[k]) if on[k] else None for k in range(6)]
        assert raw_call(e, req, need, count, max_level, sizes, parent, outs) == _abi.PE_OK, on
        for k in range(6):
            if on[k]:
                np.testing.assert_array_equal(outs[k], full[k], err_msg=str((on, k)))
    # the tables alone need neither count nor max_level
    outs = [np.full(full[0].shape, -7, dtype=np.int64)] + [None] * 5
    assert raw_call(e, req, need, None, None, sizes, parent, outs) == _abi.PE_OK
    np.testing.assert_array_equal(outs[0], full.tree_slots)
    e.close()


def test_isolation():
    inv, req, need, m = sized(2500)
    island, sizes, parent = TC.tree("racks32", 2500)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    f_req, f_need = synth.make_fit_jobs(300, 7)
    e.jobs_upload(f_req, f_need)
    e.fit_mask_run()
    rows = e.fit_mask_rows(0, 300)
    counts = e.fit_counts()
    res = e.read_residuals()
    got = e.gang_capacity_tree(req, need, counts_for(24), None, sizes, parent)
    same_tables(got, *TC.tables_of(m, island, sizes, parent))
    np.testing.assert_array_equal(e.read_residuals(), res)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    np.testing.assert_array_equal(e.fit_counts(), counts)
    e.fit_mask_run()
    np.testing.assert_array_equal(e.fit_counts(), counts)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    again = e.gang_capacity_tree(req, need, counts_for(24), None, sizes, parent)
    for a, b in zip(again, got):
        np.testing.assert_array_equal(a, b)
    e.close()
    # domains, tree, domains with different n_domains and J: the domains answers are those of an engine
    # that never made the tree call
    a, b = Engine(0), Engine(0)
    for x in (a, b):
        x.load_nodes(inv.cap, inv.used, inv.labels, island)
    req2, need2 = synth.make_fit_jobs(300, 11)
    need2 = (need2 & ~ISLAND).astype(np.uint32)
    count2 = np.resize(COUNTS, 300).astype(np.int32)
    first = [x.gang_capacity_domains(req, need, counts_for(24), sizes[0]) for x in (a, b)]
    tree = a.gang_capacity_tree(req2[:100], need2[:100], count2[:100], None, sizes, parent)
    assert tree.tree_slots.any()
    second = [x.gang_capacity_domains(req2, need2, count2, 40) for x in (a, b)]
    third = [x.gang_capacity_domains(req[:5], need[:5], counts_for(5), 200, tables=False) for x in (a, b)]
    for pair in (first, second, third):
        for u, v in zip(*pair):
            assert (u is None) == (v is None)
            if u is not None:
                np.testing.assert_array_equal(u, v)
    same = DC.tables_of(G.capacity_matrix(inv.residual(), inv.labels, req2, need2), island, 40)
    np.testing.assert_array_equal(second[0].dom_slots, same[0])
    np.testing.assert_array_equal(second[0].dom_nodes, same[1])
    a.close()
    b.close()


def test_errors():
    inv, req, need, _ = sized(1023)
    island, sizes, parent = TC.tree("racks32", 1023)
    count = counts_for(24)
    max_level = levels_for(24, 3)
    T = sum(sizes)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)

    def outputs():
        return [np.full((24, T), -7, dtype=np.int64), np.full((24, T), -7, dtype=np.int64), np.full(24, -7, dtype=np.int32),
                np.full(24, -7, dtype=np.int32), np.full(24, -7, dtype=np.int64), np.full((24, 3), -7, dtype=np.int32)]

    def refused(text, req=req, need=need, count=count, max_level=max_level, sizes=sizes, parent=parent, outs=None):
        """PE_EINVAL with `text` in the message, and no output written."""
        outs = outputs() if outs is None else outs
        assert raw_call(e, req, need, count, max_level, sizes, parent, outs) == _abi.PE_EINVAL, text
        msg = e.lib.pe_last_error(e.h).decode()
        assert text in msg, msg
        for o in outs:
            assert o is None or (o == -7).all(), text

    bad = req.copy()
    bad[5, 2] = -1
    bad[9, 0] = -7
    refused("index 22", req=bad)
    refused("index 22", req=bad, count=None, max_level=None, outs=outputs()[:2] + [None] * 4)
    zero = count.copy()
    zero[7] = 0
    zero[11] = -3
    refused("count: value below 1 at index 7", count=zero)
    refused("count: value below 1 at index 7", count=zero, outs=[None] * 5 + outputs()[5:])
    refused("count is NULL", count=None)
    for v, at in ((3, 4), (-1, 4), (2**31 - 1, 4)):
        ml = max_level.copy()
        ml[at], ml[20] = v, 3
        refused(f"max_level: value outside [0, n_levels) at index {at}", max_level=ml)
    for L in (0, 5):
        refused("n_levels", sizes=[4] * L, parent=np.zeros(16, dtype=np.int32))
    for k, v in ((0, 0), (1, 0), (2, -1), (1, _abi.PE_MAX_DOMAINS + 1)):
        s = list(sizes)
        s[k] = v
        refused(f"level_size: value outside [1, PE_MAX_DOMAINS] at index {k}", sizes=s)
    for at, v in ((3, sizes[1]), (5, -2), (sizes[0] + 2, 1), (sizes[0], -2)):
        p = parent.copy()
        p[at] = v
        p[-1] = 9
        refused(f"parent: value outside [-1, size of the level above) at index {at}", parent=p)
    refused("parent is NULL", parent=None)
    outs = outputs()
    assert e.lib.pe_gang_capacity_tree(e.h, 24, req.ctypes.data, None, count.ctypes.data, None, 3, None, parent.ctypes.data,
                                       *[o.ctypes.data for o in outs]) == _abi.PE_EINVAL
    assert b"level_size is NULL" in e.lib.pe_last_error(e.h) and all((o == -7).all() for o in outs)
    # count and max_level are not read without a selection output; every output NULL; no request; no jobs
    assert raw_call(e, req, need, zero, np.full(24, 9, dtype=np.int32), sizes, parent, outputs()[:2] + [None] * 4) == _abi.PE_OK
    assert raw_call(e, req, need, count, max_level, sizes, parent, [None] * 6) == _abi.PE_OK
    szs = np.ascontiguousarray(sizes, dtype=np.int32)
    tail = [len(sizes), szs.ctypes.data, parent.ctypes.data] + [None] * 6
    assert e.lib.pe_gang_capacity_tree(e.h, 24, None, None, None, None, *tail) == _abi.PE_EINVAL
    assert e.lib.pe_gang_capacity_tree(e.h, -1, req.ctypes.data, None, None, None, *tail) == _abi.PE_EINVAL
    assert e.lib.pe_gang_capacity_tree(e.h, 0, None, None, None, None, *tail) == _abi.PE_OK
    none = e.gang_capacity_tree(np.zeros((0, 4), dtype=np.int64), None, np.zeros(0, dtype=np.int32), None, sizes, parent)
    assert none.tree_slots.shape == (0, T) and none.level.shape == (0,) and none.feasible.shape == (0, 3)
    # the Python handle raises what the engine returns
    with pytest.raises(PlacementError) as ei:
        e.gang_capacity_tree(req, need, count, None, [sizes[0], 0, 1], None)
    assert ei.value.code == _abi.PE_EINVAL and "level_size" in str(ei.value)
    # the largest hierarchy is accepted
    top_sizes = [_abi.PE_MAX_DOMAINS] * _abi.PE_MAX_LEVELS
    ids = np.arange(_abi.PE_MAX_DOMAINS)                  # the racks in blocks of 4 as before, every block -> 0 -> 0
    top_parent = np.concatenate([np.where(ids < sizes[0], ids // 4, -1), 0 * ids, 0 * ids]).astype(np.int32)
    top = e.gang_capacity_tree(req[:2], need[:2], count[:2], None, top_sizes, top_parent, tables=False)
    ref = e.gang_capacity_tree(req[:2], need[:2], count[:2], None, sizes, parent, tables=False)
    np.testing.assert_array_equal(top.feasible[:, :2], ref.feasible[:, :2])
    np.testing.assert_array_equal(top.feasible[:, 2], ref.feasible[:, 2])
    np.testing.assert_array_equal(top.feasible[:, 3], ref.feasible[:, 2])
    e.close()
    fresh = Engine(0)
    with pytest.raises(PlacementError) as ei:
        fresh.gang_capacity_tree(req, need, count, max_level, sizes, parent)
    assert ei.value.code == _abi.PE_ESTATE
    # an inventory of no nodes: zeros and -1, whatever the arrays held
    fresh.load_nodes(np.zeros((4, 0), dtype=np.int64), np.zeros((4, 0), dtype=np.int64))
    outs = outputs()
    assert raw_call(fresh, req, need, count, max_level, sizes, parent, outs) == _abi.PE_OK
    assert not outs[0].any() and not outs[1].any() and (outs[2] == -1).all() and (outs[3] == -1).all()
    assert not outs[4].any() and not outs[5].any()
    fresh.close()
