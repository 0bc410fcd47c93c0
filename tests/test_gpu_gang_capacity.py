"""pe_gang_capacity on the GPU against the Python-integer checker (tests/gang_capacity.py): every output
of every job compared, nothing sampled."""
import numpy as np
import pytest

import gang_capacity as G
from placement import Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)


def same(got, want):
    for g, w, name in zip(got, want, ("slots", "max_node", "nodes")):
        assert g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.fixture(scope="module")
def inv3000():
    return synth.make_inventory(3000, 7)


@pytest.fixture(scope="module")
def jobs300():
    return synth.make_fit_jobs(300, 7)


@pytest.fixture(scope="module")
def want3000(inv3000, jobs300):
    return G.capacity(inv3000.residual(), inv3000.labels, *jobs300)


@pytest.fixture()
def eng3000(inv3000):
    e = Engine(0)
    e.load_nodes(inv3000.cap, inv3000.used, inv3000.labels, inv3000.island)
    yield e
    e.close()


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 257, 3000, 8193])
def test_sizes(n_nodes):
    inv = synth.make_inventory(n_nodes, 7)
    req, need = synth.make_fit_jobs(300, 7 + n_nodes)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    got = e.gang_capacity(req, need)
    same(got, G.capacity(inv.residual(), inv.labels, req, need))
    np.testing.assert_array_equal(got[2], e.fit_mask(req, need))   # nodes = the fit mask's counts
    e.close()


def test_one_job_and_one_shape(eng3000, inv3000, jobs300, want3000):
    req, need = jobs300
    for j in (0, 17, 299):
        same(eng3000.gang_capacity(req[j:j + 1], need[j:j + 1]), [w[j:j + 1] for w in want3000])
    # every job the same shape: one shape on the device, scattered to all
    got = eng3000.gang_capacity(np.repeat(req[5:6], 1000, axis=0), np.repeat(need[5:6], 1000))
    same(got, [np.repeat(w[5:6], 1000) for w in want3000])
    # shapes that recur out of order
    idx = np.array([3, 9, 3, 3, 250, 9, 0, 250, 3], dtype=np.int64)
    same(eng3000.gang_capacity(req[idx], need[idx]), [w[idx] for w in want3000])
    # need = None is need 0
    same(eng3000.gang_capacity(req[:40]), G.capacity(inv3000.residual(), inv3000.labels, req[:40], None))


def test_arithmetic_edges():
    cap, used, labels, island = G.edge_inventory()
    req, need = G.edge_shapes()
    e = Engine(0)
    e.load_nodes(cap, used, labels, island)
    got = e.gang_capacity(req, need)
    want = G.capacity(cap - used, synth.island_labels(labels, island), req, need)
    same(got, want)
    assert (got[1] == G.CAP_MAX).any() and (got[0] > np.int64(G.CAP_MAX)).any()
    e.close()


def test_special_cells():
    cap, used, labels, island = G.special_inventory()
    e = Engine(0)
    e.load_nodes(cap, used, labels, island)
    req = np.array([c[0] for c in G.SPECIAL_CASES], dtype=np.int64)
    need = np.array([c[1] for c in G.SPECIAL_CASES], dtype=np.uint32)
    slots, max_node, nodes = e.gang_capacity(req, need)
    for j, (_, _, cells) in enumerate(G.SPECIAL_CASES):
        assert (int(slots[j]), int(max_node[j]), int(nodes[j])) == (sum(cells), max(cells), sum(c >= 1 for c in cells)), j
    # each node alone: the cells themselves
    for n in range(cap.shape[1]):
        one = Engine(0)
        one.load_nodes(cap[:, n:n + 1], used[:, n:n + 1], labels[n:n + 1], island[n:n + 1])
        s, m, k = one.gang_capacity(req, need)
        cells = [c[2][n] for c in G.SPECIAL_CASES]
        assert s.tolist() == cells and m.tolist() == cells and k.tolist() == [int(c >= 1) for c in cells], n
        one.close()
    e.close()


def test_labels(eng3000, inv3000, jobs300):
    req, need = jobs300
    none = eng3000.gang_capacity(req, np.full(300, 1 << 30, dtype=np.uint32))   # a bit no node carries
    for a in none:
        assert not a.any()
    isl_need = (need | ISLAND).astype(np.uint32)
    got = eng3000.gang_capacity(req, isl_need)
    same(got, G.capacity(inv3000.residual(), inv3000.labels, req, isl_need))
    on = inv3000.island >= 0                                                    # only the island nodes count
    same(got, G.capacity(inv3000.residual()[:, on], inv3000.labels[on], req, need))
    assert got[0].any() and 0 < int(on.sum()) < 3000


def test_current_residuals(eng3000, inv3000, jobs300, want3000):
    req, need = jobs300
    e = eng3000
    same(e.gang_capacity(req, need), want3000)
    _, st = e.place_batch(synth.make_jobs(100, 7, "mixed"))
    assert (st == 0).any()
    res = e.read_residuals()
    after = e.gang_capacity(req, need)
    same(after, G.capacity(res, inv3000.labels, req, need))
    assert (after[0] < want3000[0]).any()
    e.reset_residuals()
    same(e.gang_capacity(req, need), want3000)
    # a removed slot holds nothing
    m = G.capacity_matrix(inv3000.residual(), inv3000.labels, req, need)
    slot = int(np.argmax(np.asarray(m >= 1, dtype=bool).sum(axis=0)))
    assert (m[:, slot] >= 1).any()
    e.update_nodes([slot], [_abi.PE_NODE_REMOVE])
    m[:, slot] = 0
    want = (np.array([int(sum(r)) for r in m], dtype=np.int64), np.array([int(max(r)) for r in m], dtype=np.int32),
            np.array([int(np.count_nonzero(r >= 1)) for r in m], dtype=np.int64))
    same(e.gang_capacity(req, need), want)
    same(e.gang_capacity(req, need), G.capacity(e.read_residuals(), np.where(np.arange(3000) == slot, 0, inv3000.labels),
                                                req, need))


def test_greedy_equivalence_on_device():
    inv = G.greedy_inventory()
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    for shapes, which in ((G.greedy_shapes(), 0), (G.greedy_island_shapes(), 1)):
        for req, need in shapes:
            got = e.gang_capacity([req], [need])
            same(got, G.capacity(inv.residual(), inv.labels, [req], [need]))
            limit = int(got[which][0])
            assert limit >= 2
            for count in (limit - 1, limit, limit + 1):
                e.reset_residuals()
                pods, st = e.place_greedy(*G.one_group_batch(count, req, need))
                assert (int(st[0]) == _abi.PE_JOB_PLACED) == (count <= limit), (req, need, count, limit)
                assert (pods >= 0).all() == (count <= limit)
    e.close()


@pytest.mark.parametrize("n_nodes,world", [(3000, 4), (3, 8)])
def test_shards(n_nodes, world):
    inv = synth.make_inventory(n_nodes, 7)
    req, need = synth.make_fit_jobs(300, 7)
    want = G.capacity(inv.residual(), inv.labels, req, need)
    slots = np.zeros(300, dtype=np.int64)
    nodes = np.zeros(300, dtype=np.int64)
    max_node = np.zeros(300, dtype=np.int32)
    empty = 0
    for r in range(world):
        s = Engine(0, rank=r, world_size=world, exchange=lambda b, w=world: b * w)
        s.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
        b, e = s.shard_range()
        got = s.gang_capacity(req, need)
        same(got, G.capacity(inv.residual()[:, b:e], inv.labels[b:e], req, need))
        if b == e:
            empty += 1
            assert not got[0].any() and not got[1].any() and not got[2].any()
        slots += got[0]
        nodes += got[2]
        max_node = np.maximum(max_node, got[1])
        s.close()
    same((slots, max_node, nodes), want)
    assert (empty > 0) == (world > n_nodes)


def test_isolation_from_the_staged_fit_mask(eng3000, jobs300):
    req, need = jobs300
    e = eng3000
    e.jobs_upload(req, need)
    e.fit_mask_run()
    rows = e.fit_mask_rows(0, 300)
    counts = e.fit_counts()
    other_req, other_need = synth.make_fit_jobs(500, 9)
    got = e.gang_capacity(other_req, other_need)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    np.testing.assert_array_equal(e.fit_counts(), counts)
    e.fit_mask_run()
    np.testing.assert_array_equal(e.fit_counts(), counts)
    np.testing.assert_array_equal(e.fit_mask_rows(0, 300), rows)
    same(e.gang_capacity(other_req, other_need), got)
    np.testing.assert_array_equal(e.gang_capacity(req, need)[2], counts)


def test_errors(eng3000, jobs300):
    req, need = jobs300
    bad = req.copy()
    bad[5, 2] = -1
    bad[9, 0] = -7
    with pytest.raises(PlacementError) as ei:
        eng3000.gang_capacity(bad, need)
    assert ei.value.code == _abi.PE_EINVAL and "index 22" in str(ei.value)
    fresh = Engine(0)
    with pytest.raises(PlacementError) as ei:
        fresh.gang_capacity(req, need)
    assert ei.value.code == _abi.PE_ESTATE
    fresh.close()
    for a in eng3000.gang_capacity(np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.uint32)):
        assert a.shape == (0,)
    lib, h = eng3000.lib, eng3000.h
    rq = np.ascontiguousarray(req[:8])
    p = rq.ctypes.data
    assert lib.pe_gang_capacity(h, 0, None, None, None, None, None) == _abi.PE_OK
    assert lib.pe_gang_capacity(h, 8, p, None, None, None, None) == _abi.PE_OK     # every output NULL
    assert lib.pe_gang_capacity(h, 8, None, None, None, None, None) == _abi.PE_EINVAL   # NULL req
    assert lib.pe_gang_capacity(h, -1, p, None, None, None, None) == _abi.PE_EINVAL
    full = eng3000.gang_capacity(rq)
    for k, dt in enumerate((np.int64, np.int32, np.int64)):                        # each output alone
        out = np.zeros(8, dtype=dt)
        args = [None, None, None]
        args[k] = out.ctypes.data
        assert lib.pe_gang_capacity(h, 8, p, None, *args) == _abi.PE_OK
        np.testing.assert_array_equal(out, full[k])
