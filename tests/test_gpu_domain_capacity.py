"""pe_gang_capacity_domains on the GPU against the Python-integer checker (tests/domain_capacity.py): every
cell of both tables and every selection output of every job compared, nothing sampled."""
import itertools

import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
from placement import Engine, PlacementError, _abi, select_domain, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)
COUNTS = np.array([1, 2, 3, 8, 40, 500, 5000, 2**31 - 1], dtype=np.int32)


def counts_for(J):
    return np.resize(COUNTS, J).astype(np.int32)


def same_tables(got, want_slots, want_nodes):
    assert got.dom_slots.dtype == np.int64 and got.dom_nodes.dtype == np.int64
    np.testing.assert_array_equal(got.dom_slots, want_slots, err_msg="dom_slots")
    np.testing.assert_array_equal(got.dom_nodes, want_nodes, err_msg="dom_nodes")


def same_selection(got, want_slots, count):
    dom, slots, feas = DC.select(want_slots, count)
    assert got.domain.dtype == np.int32 and got.domain_slots.dtype == np.int64 and got.feasible.dtype == np.int32
    np.testing.assert_array_equal(got.domain, dom, err_msg="domain")
    np.testing.assert_array_equal(got.domain_slots, slots, err_msg="domain_slots")
    np.testing.assert_array_equal(got.feasible, feas, err_msg="feasible")


def check(e, m, island, D, req, need, count):
    """The engine's answers (tables + selection, and the selection alone) against the cap matrix m."""
    want_slots, want_nodes = DC.tables_of(m, island, D)
    got = e.gang_capacity_domains(req, need, count, D)
    same_tables(got, want_slots, want_nodes)
    same_selection(got, want_slots, count)
    lean = e.gang_capacity_domains(req, need, count, D, tables=False)
    assert lean.dom_slots is None and lean.dom_nodes is None
    same_selection(lean, want_slots, count)
    return want_slots, want_nodes


_sized = {}


def sized(n):
    """Per shard size: the inventory, 24 job shapes and their cap matrix (no need carries the island bit, so
    the matrix is the same under every domain layout)."""
    if n not in _sized:
        inv = synth.make_inventory(n, 7)
        req, need = synth.make_fit_jobs(24, 7 + n)
        assert not (need & ISLAND).any()
        _sized[n] = (inv, req, need, G.capacity_matrix(inv.residual(), inv.labels, req, need))
    return _sized[n]


@pytest.mark.parametrize("layout", DC.LAYOUTS)
@pytest.mark.parametrize("n_nodes", [1, 1023, 1024, 1025, 2500])
def test_sizes_and_layouts(n_nodes, layout):
    inv, req, need, m = sized(n_nodes)
    island, D = DC.layout(layout, n_nodes)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    if layout == "mixed":   # removed slots too: they count nowhere
        gone = np.arange(n_nodes)[3::11]
        if len(gone):
            e.update_nodes(gone, np.full(len(gone), _abi.PE_NODE_REMOVE, dtype=np.uint8))
        island = island.copy()
        island[gone] = -1
    want_slots, _ = check(e, m, island, D, req, need, counts_for(24))
    if layout in ("racks32", "interleaved", "one", "own"):
        assert want_slots.any() and ((island >= 0) & (island < D)).all()
        # every id below n_domains: the domains add up to pe_gang_capacity's answer for need | ISLAND
        slots, _, nodes = e.gang_capacity(req, (need | ISLAND).astype(np.uint32))
        got = e.gang_capacity_domains(req, need, None, D)
        np.testing.assert_array_equal(got.dom_slots.sum(axis=1), slots)
        np.testing.assert_array_equal(got.dom_nodes.sum(axis=1), nodes)
        assert got.domain is None
        # a node of a domain carries the island bit: asking for it changes nothing
        same_tables(e.gang_capacity_domains(req, (need | ISLAND).astype(np.uint32), None, D), got.dom_slots, got.dom_nodes)
    if layout == "none":
        assert not want_slots.any()
    e.close()


def test_arithmetic_edges():
    cap, used, labels, island0 = G.edge_inventory(4096)
    req, need = G.edge_shapes(256)
    assert not (need & ISLAND).any()
    m = G.capacity_matrix(cap - used, labels, req, need)
    count = counts_for(256)
    for island, D in ((island0, 4096), ((np.arange(4096) % 7).astype(np.int32), 7)):
        e = Engine(0)
        e.load_nodes(cap, used, labels, island)
        want_slots, want_nodes = check(e, m, island, D, req, need, count)
        assert (want_slots > G.CAP_MAX).any() == (D == 7) and (want_slots == G.CAP_MAX).any() == (D == 4096)
        assert want_nodes.any()
        e.close()


def test_state_changes():
    n = 2500
    inv, req, need, m0 = sized(n)
    count = counts_for(24)
    island, D = DC.layout("racks32", n)
    island = island.copy()
    labels = inv.labels.copy()
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, labels, island)
    before, _ = check(e, m0, island, D, req, need, count)

    def now():
        return G.capacity_matrix(e.read_residuals(), synth.island_labels(labels, island), req, need)

    # placements lower the residuals
    _, st = e.place_batch(synth.make_jobs(100, 7, "mixed"))
    assert (st == 0).any()
    after, _ = check(e, now(), island, D, req, need, count)
    assert (after < before).any()
    # a node moves to another domain (the slot is rewritten: its residual is cap - used again)
    slot = int(np.argmax(np.asarray(m0 >= 1, dtype=bool).sum(axis=0)))
    old, new = int(island[slot]), (int(island[slot]) + 40) % D
    e.update_nodes([slot], [_abi.PE_NODE_SET], inv.cap[:, slot][None], inv.used[:, slot][None], labels[slot:slot + 1], [new])
    island[slot] = new
    moved, _ = check(e, now(), island, D, req, need, count)
    assert (moved[:, new] > after[:, new]).any() and (moved[:, old] <= after[:, old]).all()
    # a node is removed
    e.update_nodes([slot], [_abi.PE_NODE_REMOVE])
    island[slot], labels[slot] = -1, 0
    removed, _ = check(e, now(), island, D, req, need, count)
    assert (removed[:, new] < moved[:, new]).any()
    # a node is added: the free slot gets another node, in yet another domain
    src, dom = (slot + 1) % n, (new + 7) % D
    e.update_nodes([slot], [_abi.PE_NODE_SET], inv.cap[:, src][None], inv.used[:, src][None], inv.labels[src:src + 1], [dom])
    island[slot], labels[slot] = dom, inv.labels[src]
    check(e, now(), island, D, req, need, count)
    # residuals reset
    e.reset_residuals()
    check(e, now(), island, D, req, need, count)
    # another inventory of another size, another layout
    inv2, req2, need2, m2 = sized(1025)
    island2, D2 = DC.layout("interleaved", 1025)
    e.load_nodes(inv2.cap, inv2.used, inv2.labels, island2)
    check(e, m2, island2, D2, req2, need2, count)
    check(e, G.capacity_matrix(inv2.residual(), inv2.labels, req, need), island2, D2, req, need, count)
    e.close()


def test_selection():
    """64 equal nodes in racks of 8; rack 3 loses one node, rack 6 two."""
    GiB = G.GiB
    cap = np.tile(np.array([[8000], [64 * GiB], [8], [100 * GiB]], dtype=np.int64), (1, 64))
    island = (np.arange(64) // 8).astype(np.int32)
    e = Engine(0)
    e.load_nodes(cap, np.zeros_like(cap), np.zeros(64, dtype=np.uint32), island)
    e.update_nodes([24, 48, 49], [_abi.PE_NODE_REMOVE] * 3)
    island[[24, 48, 49]] = -1
    small, big = [1000, 8 * GiB, 1, 0], [8000, 8 * GiB, 8, 100 * GiB]     # 8 per node / 1 per node
    # equal shapes with different counts, recurring out of order, in one batch
    jobs = [(small, 1), (small, 48), (small, 49), (small, 57), (small, 64), (small, 65), (big, 8), (big, 7), (big, 9),
            (small, 49), (big, 8), (small, 1), (small, 1)]
    req = np.array([j[0] for j in jobs], dtype=np.int64)
    count = np.array([j[1] for j in jobs], dtype=np.int32)
    got = e.gang_capacity_domains(req, None, count, 8)
    assert got.dom_slots[0].tolist() == [64, 64, 64, 56, 64, 64, 48, 64]
    assert got.dom_nodes[6].tolist() == [8, 8, 8, 7, 8, 8, 6, 8] and got.dom_slots[6].tolist() == [8, 8, 8, 7, 8, 8, 6, 8]
    # best fit; ties to the smallest id; nothing holds the gang: -1 / 0 / 0
    assert got.domain.tolist() == [6, 6, 3, 0, 0, -1, 0, 3, -1, 3, 0, 6, 6]
    assert got.domain_slots.tolist() == [48, 48, 56, 64, 64, 0, 8, 7, 0, 56, 8, 48, 48]
    assert got.feasible.tolist() == [8, 8, 7, 6, 6, 0, 6, 7, 0, 7, 6, 8, 8]
    m = G.capacity_matrix(e.read_residuals(), np.where(island >= 0, ISLAND, 0).astype(np.uint32), req, None)
    check(e, m, island, 8, req, None, count)
    # more domains than the inventory uses: the empty ones are never chosen
    wide = e.gang_capacity_domains(req, None, count, 100, tables=False)
    np.testing.assert_array_equal(wide.domain, got.domain)
    np.testing.assert_array_equal(wide.feasible, got.feasible)
    # fewer: racks 4 .. 7 count nowhere
    check(e, m, island, 4, req, None, count)
    e.close()


def test_table_chunks():
    """n_domains = 65536: the device holds the tables of 85 shapes at a time, the batch has 120."""
    n, D = 1025, 65536
    inv = synth.make_inventory(n, 7)
    ids = (np.arange(n) * 63).astype(np.int32)           # ascending, up to 64512
    req = np.array([[100 * (j + 1), G.GiB, 0, 0] for j in range(120)], dtype=np.int64)
    count = counts_for(120)
    c_slots, c_nodes = DC.tables_of(G.capacity_matrix(inv.residual(), inv.labels, req, None), np.arange(n), n)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, ids)
    got = e.gang_capacity_domains(req, None, count, D)
    np.testing.assert_array_equal(got.dom_slots[:, ids], c_slots)
    np.testing.assert_array_equal(got.dom_nodes[:, ids], c_nodes)
    np.testing.assert_array_equal(got.dom_slots.sum(axis=1), c_slots.sum(axis=1))      # nothing anywhere else
    np.testing.assert_array_equal(got.dom_nodes.sum(axis=1), c_nodes.sum(axis=1))
    dom, slots, feas = DC.select(c_slots, count)                                      # ids ascend: ties keep their order
    np.testing.assert_array_equal(got.domain, np.where(dom >= 0, ids[np.maximum(dom, 0)], -1))
    np.testing.assert_array_equal(got.domain_slots, slots)
    np.testing.assert_array_equal(got.feasible, feas)
    lean = e.gang_capacity_domains(req, None, count, D, tables=False)
    for a, b in zip(lean[2:], got[2:]):
        np.testing.assert_array_equal(a, b)
    e.close()


@pytest.mark.parametrize("n_nodes", [2500, 2])
def test_shards(n_nodes):
    """Three shard contexts (n_nodes = 2: the first is empty): their tables add up to the unsharded table."""
    inv, req, need, m = sized(n_nodes)
    island, D = DC.layout("interleaved", n_nodes)        # every domain spans the shards
    count = counts_for(24)
    want_slots, want_nodes = DC.tables_of(m, island, D)
    slots = np.zeros_like(want_slots)
    nodes = np.zeros_like(want_nodes)
    empty = 0
    for r in range(3):
        s = Engine(0, rank=r, world_size=3, exchange=lambda b: b * 3)
        s.load_nodes(inv.cap, inv.used, inv.labels, island)
        b, e = s.shard_range()
        got = s.gang_capacity_domains(req, need, None, D)
        same_tables(got, *DC.tables_of(m[:, b:e], island[b:e], D))
        if b == e:
            empty += 1
            assert not got.dom_slots.any() and not got.dom_nodes.any()
        slots += got.dom_slots
        nodes += got.dom_nodes
        for tables in (True, False):                     # one shard's table must not be selected from
            with pytest.raises(PlacementError) as ei:
                s.gang_capacity_domains(req, need, count, D, tables=tables)
            assert ei.value.code == _abi.PE_EINVAL and "shard" in str(ei.value)
        s.close()
    np.testing.assert_array_equal(slots, want_slots)
    np.testing.assert_array_equal(nodes, want_nodes)
    assert empty == (1 if n_nodes == 2 else 0)
    for got, want in zip(select_domain(slots, count), DC.select(want_slots, count)):
        np.testing.assert_array_equal(got, want)
    one = Engine(0)
    one.load_nodes(inv.cap, inv.used, inv.labels, island)
    same_tables(one.gang_capacity_domains(req, need, None, D), slots, nodes)
    one.close()


def raw_call(e, req, need, count, D, outs):
    return e.lib.pe_gang_capacity_domains(e.h, req.shape[0], req.ctypes.data, None if need is None else need.ctypes.data,
                                          None if count is None else count.ctypes.data, D,
                                          *[None if o is None else o.ctypes.data for o in outs])


def test_optional_outputs():
    inv, req, need, m = sized(1023)
    island, D = DC.layout("racks32", 1023)
    count = counts_for(24)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    full = e.gang_capacity_domains(req, need, count, D)
    same_tables(full, *DC.tables_of(m, island, D))
    dtypes = (np.int64, np.int64, np.int32, np.int64, np.int32)
    for on in itertools.product((False, True), repeat=5):
        outs = [np.full(full[k].shape, -7, dtype=dtypes[k]) if on[k] else None for k in range(5)]
        assert raw_call(e, req, need, count, D, outs) == _abi.PE_OK, on
        for k in range(5):
            if on[k]:
                np.testing.assert_array_equal(outs[k], full[k], err_msg=str((on, k)))
    # the tables alone need no count
    outs = [np.full(full[0].shape, -7, dtype=np.int64), None, None, None, None]
    assert raw_call(e, req, need, None, D, outs) == _abi.PE_OK
    np.testing.assert_array_equal(outs[0], full.dom_slots)
    e.close()


def test_isolation_from_the_staged_fit_mask():
    inv, req, need, m = sized(2500)
    island, D = DC.layout("racks32", 2500)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    f_req, f_need = synth.make_fit_jobs(300, 7)
    e.jobs_upload(f_req, f_need)
    e.fit_mask_run()
    rows = e.fit_mask_rows(0, 300)
    counts = e.fit_counts()
    res = e.read_residuals()
    got = e.gang_capacity_domains(req, need, counts_for(24), D)
    same_tables(got, *DC.tables_of(m, island, D))
    np.testing.assert_array_equal(e.read_residuals(), res)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    np.testing.assert_array_equal(e.fit_counts(), counts)
    e.fit_mask_run()
    np.testing.assert_array_equal(e.fit_counts(), counts)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    again = e.gang_capacity_domains(req, need, counts_for(24), D)
    for a, b in zip(again, got):
        np.testing.assert_array_equal(a, b)
    e.close()


def test_errors():
    inv, req, need, _ = sized(1023)
    island, D = DC.layout("racks32", 1023)
    count = counts_for(24)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)

    def refused(code, text, *args, **kw):
        with pytest.raises(PlacementError) as ei:
            e.gang_capacity_domains(*args, **kw)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)

    bad = req.copy()
    bad[5, 2] = -1
    bad[9, 0] = -7
    refused(_abi.PE_EINVAL, "index 22", bad, need, count, D)
    refused(_abi.PE_EINVAL, "index 22", bad, need, None, D)
    for d in (0, -1, _abi.PE_MAX_DOMAINS + 1):
        refused(_abi.PE_EINVAL, "n_domains", req, need, count, d)
        refused(_abi.PE_EINVAL, "n_domains", req, need, None, d, tables=False)
    zero = count.copy()
    zero[7] = 0
    zero[11] = -3
    refused(_abi.PE_EINVAL, "index 7", req, need, zero, D)
    refused(_abi.PE_EINVAL, "index 7", req, need, zero, D, tables=False)
    # a selection output without count; count without one is not read
    sel = np.zeros(24, dtype=np.int32)
    assert raw_call(e, req, need, None, D, [None, None, sel, None, None]) == _abi.PE_EINVAL
    assert b"count" in e.lib.pe_last_error(e.h)
    assert raw_call(e, req, need, zero, D, [np.zeros((24, D), dtype=np.int64), None, None, None, None]) == _abi.PE_OK
    assert raw_call(e, req, need, count, D, [None] * 5) == _abi.PE_OK                     # every output NULL
    assert e.lib.pe_gang_capacity_domains(e.h, 24, None, None, None, D, None, None, None, None, None) == _abi.PE_EINVAL
    assert e.lib.pe_gang_capacity_domains(e.h, -1, req.ctypes.data, None, None, D, None, None, None, None, None) == \
        _abi.PE_EINVAL
    assert e.lib.pe_gang_capacity_domains(e.h, 0, None, None, None, D, None, None, None, None, None) == _abi.PE_OK
    none = e.gang_capacity_domains(np.zeros((0, 4), dtype=np.int64), None, np.zeros(0, dtype=np.int32), D)
    assert none.dom_slots.shape == (0, D) and none.domain.shape == (0,)
    # the largest n_domains is accepted
    top = e.gang_capacity_domains(req[:2], need[:2], count[:2], _abi.PE_MAX_DOMAINS, tables=False)
    np.testing.assert_array_equal(top.feasible, e.gang_capacity_domains(req[:2], need[:2], count[:2], D, tables=False).feasible)
    e.close()
    fresh = Engine(0)
    with pytest.raises(PlacementError) as ei:
        fresh.gang_capacity_domains(req, need, count, D)
    assert ei.value.code == _abi.PE_ESTATE
    # an inventory of no nodes: zeros and -1, whatever the arrays held
    fresh.load_nodes(np.zeros((4, 0), dtype=np.int64), np.zeros((4, 0), dtype=np.int64))
    outs = [np.full((24, 5), -7, dtype=np.int64), np.full((24, 5), -7, dtype=np.int64), np.full(24, 9, dtype=np.int32),
            np.full(24, 9, dtype=np.int64), np.full(24, 9, dtype=np.int32)]
    assert raw_call(fresh, req, need, count, 5, outs) == _abi.PE_OK
    assert not outs[0].any() and not outs[1].any() and (outs[2] == -1).all() and not outs[3].any() and not outs[4].any()
    fresh.close()
