"""pe_place_greedy_domains on the device against tests/domain_placement.py's checker (the C oracle, domain by
domain): every pod slot, every status and every residual cell, no sampling."""
import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import tree_capacity as TC
from inventory_model import Model
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
Q = [16000, 64 * GiB, 0, 0]          # a few pods per node
Q_GPU = [8000, 32 * GiB, 2, 50 * GiB]
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working state is in LDS up to here


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- trees and sizes

@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 2500])
def test_trees(eng, name, n):
    placed = failed = 0
    for level in DP.tree_levels(name, n):
        _, st, _ = DP.check_engine(eng, DP.tree_case(name, n, level))
        placed += int((st == 0).sum())
        failed += int((st == 1).sum())
    assert placed > 0 and (failed > 0 or n == 1)


# ---------------------------------------------------------------- domain sizes across the workgroup and LDS bounds

SIZES = [1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 10000]


@pytest.mark.parametrize("size", SIZES)
def test_domain_size(eng, size):
    spread = min(4 * size, 300)      # pods that fill node after node
    jobs = [(0, 5, [(spread, Q, 0), (2, Q_GPU, 1)]),
            (0, 9, [(spread, Q, 0), (min(size, 40), [500, GiB, 0, 0], 0), (1, [1, 0, 0, 0], DP.NO_LABEL)]),   # rolled back
            (0, 8, [(spread, Q, 0)]),                                       # on the nodes that came back
            (0, 5, [(2, Q_GPU, 1 | ISLAND), (0, Q, 0), (3, [0, 0, 0, 0], 0)]),
            (0, 1, [(min(3 * size, 3000), [4000, 16 * GiB, 0, 10 * GiB], 0)]),
            (1, 0, [(3, Q, 0)]),                                            # the second, small domain
            (1, 0, [(1000, Q, 0)])]
    want = DP.check_engine(eng, DP.one_level_case([size, 5], jobs, seed=size))
    assert want[1][1] == 1 and want[1][6] == 1 and (size < 64 or (want[1] == 0).sum() >= 3)


# ---------------------------------------------------------------- the active set

def test_all_domains_active(eng):
    island, level_size, parent = TC.tree("racks32", 2500)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(2500, 23), island)
    jobs = [(d, d % 3, [(1 + d % 7, Q, 0), (d % 2, Q_GPU, 1)]) for d in range(level_size[0])]
    jobs += [(d, 1, [(200, Q, 0)]) for d in range(0, level_size[0], 5)]
    batch, dom = DP.make_batch(jobs)
    want = DP.check_engine(eng, DP.Case(cap, used, labels, island, level_size, parent, 0, batch, dom))
    assert (want[1] == 0).any() and (want[1] == 1).any()


def test_one_active_domain_and_one_without_nodes(eng):
    # "permuted" uses half of its leaf ids: leaf `empty` has no node
    island, level_size, parent = TC.tree("permuted", 2500)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(2500, 23), island)
    dom0 = DP.dom_level(island, 0, level_size, parent)
    full = int(dom0[0])
    empty = next(k for k in range(level_size[0]) if not (dom0 == k).any())
    for jobs in ([(full, 0, [(5, Q, 0)]), (full, 3, [(500, Q, 0)]), (full, 0, [])],
                 [(empty, 0, [(1, Q, 0)]), (empty, 0, [(0, Q, 0)]), (empty, 0, []), (empty, 7, [(1, [0, 0, 0, 0], 0)])]):
        batch, dom = DP.make_batch(jobs)
        want = DP.check_engine(eng, DP.Case(cap, used, labels, island, level_size, parent, 0, batch, dom))
        if jobs[0][0] == empty:
            assert want[1].tolist() == [1, 0, 0, 1] and (want[0] == -1).all()


def test_largest_level_with_200_jobs(eng):
    n = 3000
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 65536, n).astype(np.int32)
    ids[:600] = ids[0]                                   # one crowded leaf among the sparse ones
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 29), ids)
    doms = np.concatenate([ids[rng.integers(0, n, 150)], rng.integers(0, 65536, 48), [0, 65535]])
    jobs = [(int(d), int(i % 4), [(1 + i % 5, Q, 0)] + ([(2, [500, GiB, 0, 0], 0)] if i % 3 == 0 else []))
            for i, d in enumerate(doms)]
    assert len(jobs) == 200
    batch, dom = DP.make_batch(jobs)
    want = DP.check_engine(eng, DP.Case(cap, used, labels, island, [65536], None, 0, batch, dom))
    assert (want[1] == 0).any() and (want[1] == 1).any()


# ---------------------------------------------------------------- counts

def test_counts(eng):
    jobs = [(0, 9, [(100000, [0, 0, 0, 0], 0)]),                        # every pod at once, one node
            (0, 8, [(100000, [0, 0, 0, 0], 1), (3, Q, 0)]),             # ... on the best node that has label bit 0
            (1, 5, [(2, Q_GPU, 1 | ISLAND)]),                           # an island group: one node takes both, if one can
            (1, 5, [(9, Q_GPU, 1 | ISLAND)]),                           # 18 GPUs on one node: fits no node
            (1, 5, [(3, [2**62, 0, 0, 0], ISLAND)]),                    # 3 x 2^62 overflows int64: fits nowhere
            (1, 3, [(1, [500, GiB, 0, 0], ISLAND)])]
    case = DP.one_level_case([40, 7], jobs, seed=77)
    want = DP.check_engine(eng, case)
    assert want[1].tolist() == [0, 0, want[1][2], 1, 1, 0] and len(set(want[0][:100000].tolist())) == 1
    # a gang one pod larger than its domain holds: the capacity says how many, the placement agrees
    res = eng.read_residuals()
    tc = eng.gang_capacity_tree(np.array([Q], dtype=np.int64), None, None, None, case.level_size, None)
    for d in (0, 1):
        s = int(tc.tree_slots[0, d])
        for count, status in ((s + 1, 1), (s, 0)):
            batch, dom = DP.make_batch([(d, 0, [(count, Q, 0)])])
            c = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, None, 0, batch, dom)
            before = eng.read_residuals()
            w = DP.check_engine(eng, c, load=False)
            assert w[1].tolist() == [status]
            if status:
                assert np.array_equal(eng.read_residuals(), before)
    assert not np.array_equal(eng.read_residuals(), res)


def test_overflowing_island_after_a_placed_group(eng):
    """An island product that overflows after an earlier group took pods rolls that group back, and a request no
    node holds fails at the first decision."""
    jobs = [(0, 4, [(3, Q, 0), (3, [2**62, 0, 0, 0], ISLAND)]),
            (0, 3, [(3, Q, 0)]),
            (1, 7, [(5, [2**40, 0, 0, 0], 0)])]
    want = DP.check_engine(eng, DP.one_level_case([40, 7], jobs, seed=78))
    assert want[1].tolist() == [1, 0, 1]


# ---------------------------------------------------------------- capacity round trip on the device

@pytest.mark.parametrize("name", ["racks32", "four", "permuted"])
def test_capacity_round_trip(eng, name):
    n = 1025
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    eng.load_nodes(cap, used, labels, island)
    req = np.array([Q, Q_GPU, Q, Q, Q], dtype=np.int64)
    need = np.array([0, 1, 0, 0, 0], dtype=np.uint32)
    count = np.array([1, 10, 60, 500, 2000], dtype=np.int32)
    tc = eng.gang_capacity_tree(req, need, count, None, level_size, parent, tables=False)
    assert (tc.level >= 0).sum() >= 3 and len(set(tc.level[tc.level >= 0].tolist())) >= 2
    for j in np.nonzero(tc.level >= 0)[0]:
        level, d, s = int(tc.level[j]), int(tc.domain[j]), int(tc.domain_slots[j])
        assert s >= count[j]
        for pods, status in ((s + 1, 1), (s, 0)):
            eng.reset_residuals()
            before = eng.read_residuals()
            batch, dom = DP.make_batch([(d, 0, [(pods, req[j].tolist(), int(need[j]))])])
            w = DP.check_engine(eng, DP.Case(cap, used, labels, island, level_size, parent, level, batch, dom), load=False)
            assert w[1].tolist() == [status]
            assert np.array_equal(eng.read_residuals(), before) == bool(status)


# ---------------------------------------------------------------- state

def test_state_across_calls():
    n = 1200
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 51)
    model = Model(inv.residual(), inv.labels, island)
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    fit_req, fit_need = synth.make_fit_jobs(64, 9)
    e.jobs_upload(fit_req, fit_need)                       # staged before all of it

    def same_state():
        assert np.array_equal(e.read_residuals(), model.res)
        e.fit_mask_run()
        assert np.array_equal(e.fit_counts(), model.fit(fit_req, fit_need)[1])

    def domains_call(level, seed, sizes=level_size, par=parent):
        batch, dom = DP.job_mix(model.res, model.labels, model.island, level, sizes, par, seed)
        want = DP.place(model.res, model.labels, model.island, batch, dom, level, sizes, par)
        s0 = e.stats()
        pods, st = e.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                          batch.group_need, dom, level, sizes, par)
        s1 = e.stats()
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1])
        model.res = want[2]
        poff = DP.pod_offsets(batch.group_count)
        placed = [j for j in range(len(st)) if st[j] == 0]
        want_stats = dict(s0)
        want_stats["jobs_placed"] += len(placed)
        want_stats["jobs_failed"] += len(st) - len(placed)
        want_stats["pods_placed"] += sum(poff[batch.job_group_off[j + 1]] - poff[batch.job_group_off[j]] for j in placed)
        assert s1 == want_stats                            # nothing else in pe_stats moves
        same_state()
        return st

    same_state()
    assert (domains_call(0, 1) == 0).any()
    greedy = synth.make_jobs(60, 7, "mixed")               # unconstrained: reads the host mirror
    pods, st = e.place_batch(greedy)
    w_pods, w_st, _ = model.place(greedy)
    assert np.array_equal(pods, w_pods) and np.array_equal(st, w_st) and (st == 0).any()
    same_state()
    domains_call(1, 2)                                     # a second call without a reset, another level
    donor = synth.make_inventory(3, 52, 0.5)
    upd = (np.array([5, 40, 700]), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # node 5 moves to rack 30, node 40 goes, node 700 joins rack 2
    e.update_nodes(*upd)
    model.update(upd)
    same_state()
    domains_call(0, 3)
    e.update_nodes(np.array([40]), np.array([PE_NODE_SET], dtype=np.uint8), np.ascontiguousarray(donor.cap.T[:1]),
                   np.ascontiguousarray(donor.used.T[:1]), donor.labels[:1].copy(), np.array([1], dtype=np.int32))
    model.update((np.array([40]), np.array([PE_NODE_SET], dtype=np.uint8), np.ascontiguousarray(donor.cap.T[:1]),
                  np.ascontiguousarray(donor.used.T[:1]), donor.labels[:1].copy(), np.array([1], dtype=np.int32)))
    domains_call(0, 4)                                     # the node that was added takes part
    e.reset_residuals()
    model.reset()
    same_state()
    domains_call(2, 5)
    # another hierarchy over the same inventory: nothing of the first one was kept
    sizes2 = [level_size[0], 3]
    parent2 = (np.arange(level_size[0]) % 4 - 1).astype(np.int32)     # every fourth rack in no zone
    domains_call(1, 6, sizes2, parent2)
    domains_call(0, 7, [level_size[0]], None)
    pods, st = e.place_batch(greedy)
    w_pods, w_st, _ = model.place(greedy)
    assert np.array_equal(pods, w_pods) and np.array_equal(st, w_st)
    # reload: another size, other islands
    island3, sizes3, parent3 = TC.tree("four", 700)
    inv3 = synth.make_inventory(700, 53)
    e.load_nodes(inv3.cap, inv3.used, inv3.labels, island3)
    model = Model(inv3.residual(), inv3.labels, island3)
    e.jobs_upload(fit_req, fit_need)
    same_state()
    for level in range(4):
        domains_call(level, 8 + level, sizes3, parent3)
    e.close()


def test_alternating_with_the_capacity_calls():
    n = 1025
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 61)
    labels = synth.island_labels(inv.labels, island)
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    a.load_nodes(inv.cap, inv.used, inv.labels, island)
    req, need = synth.make_fit_jobs(40, 11)
    count = np.resize(np.array([1, 8, 40, 200, 1000], dtype=np.int32), 40)
    zero = np.zeros_like(inv.cap)
    for step in range(3):
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, labels, island, step, level_size, parent, 90 + step)
        want = DP.place(res, labels, island, batch, dom, step, level_size, parent)
        pods, st = a.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                          batch.group_need, dom, step, level_size, parent)
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1])
        assert np.array_equal(a.read_residuals(), want[2]) and (want[2] >= 0).all()
        b.load_nodes(want[2], zero, inv.labels, island)    # the same residuals, loaded
        for x, y in zip(a.gang_capacity(req, need), b.gang_capacity(req, need)):
            assert np.array_equal(x, y)
        for x, y in zip(a.gang_capacity_domains(req, need, count, level_size[0]),
                        b.gang_capacity_domains(req, need, count, level_size[0])):
            assert np.array_equal(x, y)
        for x, y in zip(a.gang_capacity_tree(req, need, count, None, level_size, parent),
                        b.gang_capacity_tree(req, need, count, None, level_size, parent)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.read_residuals(), want[2])
    a.close()
    b.close()


# ---------------------------------------------------------------- refusals

SENTINEL = -77


def raw(e, off, pri, cnt, req, need, dom, level, sizes, parent, pods, st, n_jobs=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(off, np.int32), arr(pri, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32),
            arr(dom, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    # the jobs: from the offsets, or -- for a call without them -- from the priorities
    J = n_jobs if n_jobs is not None else len(keep[0]) - 1 if keep[0] is not None else len(keep[1])
    L = len(keep[6]) if n_levels is None else n_levels
    rc = e.lib.pe_place_greedy_domains(e.h, J, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                       ptr(keep[5]), level, L, ptr(keep[6]), ptr(keep[7]), ptr(pods), ptr(st))
    return rc, e.lib.pe_last_error(e.h).decode()


def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    off, pri, cnt = [0, 1, 3], [0, 1], [2, 1, 3]
    req = np.array([Q, Q_GPU, Q], dtype=np.int64)
    need, dom = [0, 1, 0], [1, 2]
    pods = np.full(6, SENTINEL, dtype=np.int32)
    st = np.full(2, SENTINEL, dtype=np.int32)
    good = dict(off=off, pri=pri, cnt=cnt, req=req, need=need, dom=dom, level=0, sizes=sizes, parent=parent)

    def refused(code, text, **change):
        args = dict(good, **change)
        extra = {k: args.pop(k) for k in ("n_jobs", "n_levels", "no_pods", "no_st") if k in args}
        rc, msg = raw(e, pods=None if extra.pop("no_pods", False) else pods, st=None if extra.pop("no_st", False) else st,
                      **args, **extra)
        assert rc == code and text in msg, (rc, msg, change)
        assert (pods == SENTINEL).all() and (st == SENTINEL).all()

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before = e.read_residuals()
    E = _abi.PE_EINVAL
    bad_req = req.copy()
    bad_req[1, 2] = -1
    # what pe_place_greedy refuses
    refused(E, "negative request at index 6", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "job_group_off[0]", off=[1, 1, 3])
    refused(E, "not monotonic", off=[0, 2, 1])
    refused(E, "n_jobs < 0", n_jobs=-1)
    for name in ("off", "pri", "cnt", "req"):
        refused(E, "is NULL", **{name: None})
    refused(E, "out_pod_node is NULL", no_pods=True)
    refused(E, "out_job_status is NULL", no_st=True)
    # the domains
    refused(E, "job_domain is NULL", dom=None)
    refused(E, "job_domain: value outside [0, level_size[level]) at index 1", dom=[9, 10])
    refused(E, "job_domain: value outside [0, level_size[level]) at index 0", dom=[-1, 10])
    refused(E, "at index 0", dom=[3, 0], level=1)          # a leaf id that level 1 does not have
    refused(E, "level outside", level=-1)
    refused(E, "level outside", level=3)
    # what tree_plan_build refuses
    refused(E, "n_levels outside", n_levels=0)
    refused(E, "n_levels outside", n_levels=5, sizes=sizes + [1, 1])
    refused(E, "level_size is NULL", sizes=None, n_levels=3)
    refused(E, "level_size: value outside [1, PE_MAX_DOMAINS] at index 1", sizes=[10, 0, 1])
    refused(E, "level_size: value outside [1, PE_MAX_DOMAINS] at index 0", sizes=[65537, 3, 1])
    refused(E, "parent is NULL", parent=None)
    bad_parent = np.array(parent).copy()
    bad_parent[4] = 3
    refused(E, "parent: value outside [-1, size of the level above) at index 4", parent=bad_parent)
    bad_parent[4] = -2
    refused(E, "at index 4", parent=bad_parent)
    assert np.array_equal(e.read_residuals(), before)
    # the same arguments unchanged are accepted, and the sentinels go
    rc, msg = raw(e, pods=pods, st=st, **good)
    assert rc == _abi.PE_OK, msg
    assert (st != SENTINEL).all() and (pods != SENTINEL).all()
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.place_greedy_domains(off, pri, cnt, req, need, dom, 7, sizes, parent)
    assert ei.value.code == E and "level" in str(ei.value)
    e.close()


def test_sharded_context_is_refused():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 71)
    for r in range(2):
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(inv.cap, inv.used, inv.labels, island)
        before = s.read_residuals()
        pods = np.full(2, SENTINEL, dtype=np.int32)
        st = np.full(1, SENTINEL, dtype=np.int32)
        rc, msg = raw(s, [0, 1], [0], [2], np.array([Q], dtype=np.int64), [0], [0], 0, sizes, parent, pods, st)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert (pods == SENTINEL).all() and (st == SENTINEL).all() and np.array_equal(s.read_residuals(), before)
        s.close()


def test_no_jobs(eng):
    n = 300
    island, sizes, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 71)
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
    before = eng.read_residuals()
    stats = eng.stats()
    rc, msg = raw(eng, None, None, None, None, None, None, 1, sizes, parent, None, None, n_jobs=0)
    assert rc == _abi.PE_OK, msg
    pods, st = eng.place_greedy_domains([0], [], [], np.zeros((0, 4), dtype=np.int64), None, np.zeros(0, dtype=np.int32), 0,
                                        sizes, parent)
    assert pods.shape == (0,) and st.shape == (0,)
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    # jobs without pods: all placed, nothing moves
    pods, st = eng.place_greedy_domains([0, 0, 1], [0, 0], [0], np.array([Q], dtype=np.int64), None, [0, 9], 0, sizes, parent)
    assert pods.shape == (0,) and st.tolist() == [0, 0] and np.array_equal(eng.read_residuals(), before)
