"""The three gang-capacity calls in turn on ONE engine: pe_gang_capacity_domains and pe_gang_capacity_tree
are one host path over one set of buffers (and share the shapes' with pe_gang_capacity), so calls of
different shapes -- few and many columns, one and three levels, with and without tables, with and without
a selection -- must each size and fill what they use.  Every answer against the Python-integer checkers
(tests/gang_capacity.py, domain_capacity.py, tree_capacity.py), integer and exact."""
import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
import tree_capacity as TC
from placement import Engine, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)
COUNTS = np.array([1, 8, 40, 200, 1000, 5000, 30000, 2**31 - 1], dtype=np.int32)


def test_alternating_calls_on_one_engine():
    n = 1025                                              # one full node block and one node
    inv = synth.make_inventory(n, 7)
    req, need = synth.make_fit_jobs(24, 7 + n)
    assert not (need & ISLAND).any()                      # the cap matrix is the same under every call
    m = G.capacity_matrix(inv.residual(), inv.labels, req, need)
    island, sizes, parent = TC.tree("racks32", n)         # 33 racks -> 9 blocks -> 1 root
    assert sizes == [33, 9, 1]
    count = np.resize(COUNTS, 24).astype(np.int32)
    max_level = ((np.arange(24) // len(COUNTS) + np.arange(24)) % 3).astype(np.int32)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)

    def whole():
        slots, max_node, nodes = e.gang_capacity(req, need)
        np.testing.assert_array_equal(slots, m.sum(axis=1).astype(np.int64))
        np.testing.assert_array_equal(max_node, m.max(axis=1).astype(np.int32))
        np.testing.assert_array_equal(nodes, np.asarray(m >= 1, dtype=bool).sum(axis=1))
        assert slots.any()

    def domains8():                                       # the racks past the eighth count nowhere
        got = e.gang_capacity_domains(req, need, count, 8)
        want_slots, want_nodes = DC.tables_of(m, island, 8)
        np.testing.assert_array_equal(got.dom_slots, want_slots)
        np.testing.assert_array_equal(got.dom_nodes, want_nodes)
        for a, b in zip((got.domain, got.domain_slots, got.feasible), DC.select(want_slots, count)):
            assert a.shape == b.shape
            np.testing.assert_array_equal(a, b)
        assert (got.domain >= 0).any() and (got.domain < 0).any()

    def tree3():
        got = e.gang_capacity_tree(req, need, count, max_level, sizes, parent)
        want_slots, want_nodes = TC.tables_of(m, island, sizes, parent)
        np.testing.assert_array_equal(got.tree_slots, want_slots)
        np.testing.assert_array_equal(got.tree_nodes, want_nodes)
        for a, b in zip(got[2:], TC.select(want_slots, count, sizes, max_level)):
            assert a.shape == b.shape
            np.testing.assert_array_equal(a, b)
        assert len(set(got.level.tolist())) == 4          # every level and none

    def domains65536():                                   # the widest table, two shapes, only the answers cross
        got = e.gang_capacity_domains(req[:2], need[:2], count[1:3], 65536, tables=False)
        assert got.dom_slots is None and got.dom_nodes is None
        want_slots, _ = DC.tables_of(m[:2], island, 65536)
        assert not want_slots[:, 33:].any()
        for a, b in zip((got.domain, got.domain_slots, got.feasible), DC.select(want_slots, count[1:3])):
            assert a.shape == b.shape
            np.testing.assert_array_equal(a, b)
        assert (got.feasible > 0).any()

    def tree1():                                          # one level, no count: the tables alone
        got = e.gang_capacity_tree(req, need, None, None, sizes[:1], None)
        want_slots, want_nodes = DC.tables_of(m, island, sizes[0])
        np.testing.assert_array_equal(got.tree_slots, want_slots)
        np.testing.assert_array_equal(got.tree_nodes, want_nodes)
        assert got.level is None and got.domain is None and got.domain_slots is None and got.feasible is None

    for call in (whole, domains8, tree3, domains65536, tree1, whole, domains8, tree3):
        call()
    e.close()
