"""pe_gang_fit_domains on the device against tests/gang_fit.py's checker: every fits, fail_group, pods and first
cell, no sampling; the placement call's own verdict on sampled pairs; and that the call changes nothing."""
import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import gang_fit as GF
import tree_capacity as TC
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
Q = [16000, 64 * GiB, 0, 0]          # a few pods per node
Q_GPU = [8000, 32 * GiB, 2, 50 * GiB]
Q_BIG = [96000, 0, 0, 0]             # a pod for every fourth node or so: a domain's slots stay small
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working copy is in LDS up to here


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def slots_of(res, nodes, q):
    """Pods of request q (no need) that `nodes` hold: the capacity rule in numpy, for sizing the cases."""
    cap = np.full(len(nodes), 2**31 - 1, dtype=np.int64)
    for d in range(4):
        if q[d] > 0:
            cap = np.minimum(cap, np.where(res[d][nodes] >= 0, res[d][nodes] // q[d], 0))
    return int(cap.sum()), int(cap.max(initial=0))


def with_jobs(case, jobs):
    case.batch, case.job_domain = DP.make_batch([(0, 0, groups) for groups in jobs])
    return case


# ---------------------------------------------------------------- trees and sizes

@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 2500])
def test_trees(eng, name, n):
    fitting = failing = 0
    for level in DP.tree_levels(name, n):
        case, pj, pd = GF.pairs_case(name, n, level)
        fits, _, _, _ = GF.check_engine(eng, case, pj, pd, python=n <= 257)
        fitting += int(fits.sum())
        failing += int((fits == 0).sum())
    assert fitting > 0 and (failing > 0 or n == 1)


# ---------------------------------------------------------------- domain sizes across the workgroup and LDS bounds

SIZES = [1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 1023, 1024, 1025, 2049, 4097, 10000]


@pytest.mark.parametrize("size", SIZES)
def test_domain_size(eng, size):
    """Two jobs on the large domain in one call, the one that does not fit first: it takes every slot of the domain
    before it fails, and the one after it needs every slot again -- a working copy that is not refreshed shows."""
    case = DP.one_level_case([size, 5], [], seed=size)
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    s, _ = slots_of(case.residual(), np.nonzero(dom == 0)[0], Q_BIG)
    assert s > 0 or size == 1
    jobs = [[(s, Q_BIG, 0), (1, [1, 0, 0, 0], DP.NO_LABEL)],                 # all the slots, then no fit
            [(s, Q_BIG, 0), (2, [0, GiB, 0, 0], 0)],                         # all the slots again, then memory only
            [(s + 1, Q_BIG, 0)],                                            # one pod too many
            [(2, Q_GPU, 1 | ISLAND), (0, Q, 0), (3, [0, 0, 0, 0], 0), (min(3 * size, 3000), [4000, 16 * GiB, 0, 10 * GiB], 0)]]
    with_jobs(case, jobs)
    pj = np.array([0, 1, 2, 1, 0, 1, 3, 3, 2], dtype=np.int32)
    pd = np.array([0, 0, 0, 0, 1, 1, 0, 1, 1], dtype=np.int32)
    fits, fail, pods, first = GF.check_engine(eng, case, pj, pd)
    assert (fits[0], fail[0], pods[0]) == (0, 1, s)
    assert (fits[1], fail[1], pods[1]) == (1, -1, s + 2) and fits[3] == 1
    assert (fits[2], fail[2], pods[2]) == (0, 0, s)
    assert first[:3].tolist() == [-1, 1, -1]


def test_many_pairs_on_one_small_domain_and_three_on_a_large_one(eng):
    """2000 pairs on a 64-node domain (63 units of 32) and 3 on a 3000-node domain, both kernels in one call."""
    case = DP.one_level_case([64, 3000], [], seed=12)
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    s0, _ = slots_of(case.residual(), np.nonzero(dom == 0)[0], Q)
    s1, _ = slots_of(case.residual(), np.nonzero(dom == 1)[0], Q_BIG)
    jobs = [[(s0 + k - 10, Q, 0)] + ([(1, [500, GiB, 0, 0], 0)] if k % 3 == 0 else []) for k in range(20)]   # around the slots
    jobs += [[(s1, Q_BIG, 0), (1, [1, 0, 0, 0], DP.NO_LABEL)], [(s1, Q_BIG, 0)], [(s1 + 1, Q_BIG, 0)]]
    with_jobs(case, jobs)
    rng = np.random.default_rng(5)
    pj = np.concatenate([rng.integers(0, 20, 2000), [20, 21, 22]]).astype(np.int32)
    pd = np.concatenate([np.zeros(2000), [1, 1, 1]]).astype(np.int32)
    order = rng.permutation(2003)
    order = np.concatenate([order[order != 2001], [2001]])                 # the large domain's fitting job after the failing one
    fits, fail, pods, _ = GF.check_engine(eng, case, pj[order], pd[order])
    small = pd[order] == 0
    assert 0 < fits[small].sum() < 2000
    assert fits[~small].tolist().count(1) == 1 and sorted(pods[~small].tolist()) == [s1, s1, s1]


def test_largest_level_with_200_pairs(eng):
    n = 3000
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 65536, n).astype(np.int32)
    ids[:600] = ids[0]                                   # one crowded leaf among the sparse ones
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 29), ids)
    jobs = [[(1 + i % 5, Q, 0)] + ([(2, [500, GiB, 0, 0], 0)] if i % 3 == 0 else []) for i in range(50)]
    batch, _ = DP.make_batch([(0, 0, g) for g in jobs])
    case = DP.Case(cap, used, labels, island, [65536], None, 0, batch, None)
    pd = np.concatenate([ids[rng.integers(0, n, 150)], rng.integers(0, 65536, 48), [0, 65535]]).astype(np.int32)
    pj = rng.integers(0, 50, 200).astype(np.int32)
    fits, _, _, _ = GF.check_engine(eng, case, pj, pd)
    assert fits.any() and not fits.all()


# ---------------------------------------------------------------- edge shapes

def test_edge_shapes(eng):
    case = DP.one_level_case([40, 7, 0], [], seed=77)                      # domain 2 has no node
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    res = case.residual()
    s, _ = slots_of(res, np.nonzero(dom == 0)[0], Q)
    _, one = slots_of(res, np.nonzero(dom == 1)[0], [500, GiB, 0, 0])       # what domain 1's best node holds
    jobs = [[],                                                             # 0: no groups
            [(0, Q, 0), (0, Q_GPU, ISLAND)],                                # 1: zero-count groups only
            [(100000, [0, 0, 0, 0], 0)],                                    # 2: every pod at once
            [(s, Q, 0)],                                                    # 3: exactly the domain's slots
            [(s + 1, Q, 0)],                                                # 4: one pod larger
            [(one, [500, GiB, 0, 0], ISLAND)],                              # 5: an island group one node holds
            [(2, Q, 0), (one + 1, [500, GiB, 0, 0], ISLAND)],               # 6: ... and one no node holds
            [(3, Q, 0), (3, [2**62, 0, 0, 0], ISLAND)],                     # 7: 3 x 2^62 overflows int64
            [(0, Q, 0), (2, Q, 0), (0, Q, 0), (1, [1, 0, 0, 0], DP.NO_LABEL)],   # 8: fails at its fourth group
            [(1, Q, 0)]]                                                    # 9: in no pair
    with_jobs(case, jobs)
    pj = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 1, 2, 3, 3, 4, 3, 5, 6], dtype=np.int32)
    pd = np.array([2, 2, 2, 0, 0, 1, 1, 1, 1, 0, 1, 1, 2, 0, 0, 0, 1, 1], dtype=np.int32)
    fits, fail, pods, first = GF.check_engine(eng, case, pj, pd, python=False)
    assert fits[:9].tolist() == [1, 1, 0, 1, 0, 1, 0, 0, 0]
    assert fail[:9].tolist() == [-1, -1, 0, -1, 0, -1, 1, 1, 3]
    assert pods[:9].tolist() == [0, 0, 0, s, s, one, 2, 3, 2]
    assert (fits[11], pods[11]) == (1, 100000) and (fits[12], fail[12], pods[12]) == (0, 0, 0)
    assert first.tolist() == [0, 1, 11, 3, -1, 5, -1, -1, -1, -1]
    # the same call asked for less: only the selection, only the tables, nothing at all
    b = case.batch
    args = (b.job_group_off, b.group_count, b.group_req, b.group_need, pj, pd, 0, case.level_size, None)
    sel = eng.gang_fit_domains(*args, tables=False)
    assert sel.fits is None and sel.fail_group is None and sel.pods is None and np.array_equal(sel.first, first)
    tab = eng.gang_fit_domains(*args, first=False)
    assert tab.first is None and np.array_equal(tab.fits, fits) and np.array_equal(tab.fail_group, fail)
    assert np.array_equal(tab.pods, pods)
    none = eng.gang_fit_domains(*args, tables=False, first=False)
    assert none == (None, None, None, None)
    # one P-sized answer at a time
    jgo, cnt, req, need = (np.ascontiguousarray(x) for x in (b.job_group_off, b.group_count, b.group_req, b.group_need))
    sizes = np.array(case.level_size, dtype=np.int32)
    for which, want in ((0, fits), (1, fail), (2, pods)):
        outs = [np.full(len(pj), 77, dtype=t) for t in (np.uint8, np.int32, np.int64)]
        ptrs = [o.ctypes.data if k == which else None for k, o in enumerate(outs)]
        rc = eng.lib.pe_gang_fit_domains(eng.h, len(jobs), jgo.ctypes.data, cnt.ctypes.data, req.ctypes.data, need.ctypes.data,
                                         len(pj), pj.ctypes.data, pd.ctypes.data, 0, 1, sizes.ctypes.data, None, *ptrs, None)
        assert rc == 0 and np.array_equal(outs[which], want)
        assert all((o == 77).all() for k, o in enumerate(outs) if k != which)
    # no need array: 0 for every group (the island groups become plain ones)
    plain = eng.gang_fit_domains(b.job_group_off, b.group_count, b.group_req, None, pj, pd, 0, case.level_size, None)
    zero = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, None, 0,
                   synth.JobBatch(b.job_group_off, b.priority, b.group_count, b.group_req, np.zeros_like(b.group_need), b.kind),
                   case.job_domain)
    want = GF.answers(res, case.labels, case.island, zero.batch, pj, pd, 0, case.level_size, None)
    assert all(np.array_equal(x, y) for x, y in zip(plain[:3], want))


def test_no_pairs_and_no_jobs(eng):
    case = DP.tree_case("racks32", 300, 0)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before, stats = eng.read_residuals(), eng.stats()
    b = case.batch
    none = np.zeros(0, dtype=np.int32)
    got = eng.gang_fit_domains(b.job_group_off, b.group_count, b.group_req, b.group_need, none, none, 1, case.level_size, case.parent)
    assert got.fits.shape == got.fail_group.shape == got.pods.shape == (0,)
    assert got.first.tolist() == [-1] * (len(b.job_group_off) - 1)
    got = eng.gang_fit_domains([0], [], np.zeros((0, 4), dtype=np.int64), None, none, none, 0, case.level_size, case.parent)
    assert got.first.shape == (0,) and got.fits.shape == (0,)
    sizes = np.array(case.level_size, dtype=np.int32)
    par = np.ascontiguousarray(case.parent, dtype=np.int32)
    rc = eng.lib.pe_gang_fit_domains(eng.h, 0, None, None, None, None, 0, None, None, 2, len(sizes), sizes.ctypes.data,
                                     par.ctypes.data, None, None, None, None)
    assert rc == _abi.PE_OK
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats


# ---------------------------------------------------------------- the placement's own verdict

@pytest.mark.parametrize("name,level", [("racks32", 0), ("four", 1), ("permuted", 0), ("orphans", 1), ("racks32", 2)])
def test_agrees_with_the_placement(name, level):
    """On a freshly loaded engine per pair, place_greedy_domains with that job alone in that domain returns PLACED
    iff out_fits, and then places out_pods pods."""
    n = 1025
    case, pj, pd = GF.pairs_case(name, n, level)
    e = Engine(0)
    e.load_nodes(case.cap, case.used, case.labels, case.island)
    b = case.batch
    got = e.gang_fit_domains(b.job_group_off, b.group_count, b.group_req, b.group_need, pj, pd, level, case.level_size, case.parent)
    rng = np.random.default_rng(level)
    sample = np.concatenate([np.nonzero(got.fits == 0)[0][:15], rng.permutation(len(pj))[:25]])
    assert len(sample) <= 40
    seen = set()
    for p in sample:
        e.load_nodes(case.cap, case.used, case.labels, case.island)
        before = e.read_residuals()
        one, dom = DP.make_batch([(int(pd[p]), 0, GF.job_groups(b, int(pj[p])))])
        pods, st = e.place_greedy_domains(one.job_group_off, one.priority, one.group_count, one.group_req, one.group_need,
                                          dom, level, case.level_size, case.parent)
        assert int(st[0]) == 1 - int(got.fits[p])
        seen.add(int(st[0]))
        if st[0] == 0:
            assert (pods >= 0).all() and len(pods) == int(got.pods[p])
        else:
            assert np.array_equal(e.read_residuals(), before)
    assert seen == {0, 1}
    e.close()


# ---------------------------------------------------------------- read-only

def test_read_only_across_calls():
    n = 1200
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 51)
    labels = synth.island_labels(inv.labels, island)
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    fit_req, fit_need = synth.make_fit_jobs(64, 9)
    for e in (a, b):
        e.load_nodes(inv.cap, inv.used, inv.labels, island)
        e.jobs_upload(fit_req, fit_need)                   # staged before all of it
    state = {"island": np.array(island), "labels": labels, "sizes": level_size, "parent": parent}

    def fit_call(level, seed):
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, state["labels"], state["island"], level, state["sizes"], state["parent"], seed)
        case = DP.Case(None, None, state["labels"], state["island"], list(state["sizes"]), state["parent"], level, batch, dom)
        pj, pd = GF.pair_mix(case, seed)
        stats = a.stats()
        want = GF.answers(res, state["labels"], state["island"], batch, pj, pd, level, state["sizes"], state["parent"])
        got = a.gang_fit_domains(batch.job_group_off, batch.group_count, batch.group_req, batch.group_need, pj, pd, level,
                                 state["sizes"], state["parent"])
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], want))
        assert np.array_equal(got.first, GF.first_of(pj, want[0], len(dom)))
        assert got.fits.any() and not got.fits.all()
        assert a.stats() == stats                          # pe_stats as before the call
        assert np.array_equal(a.read_residuals(), res)     # bit-equal
        assert np.array_equal(b.read_residuals(), res)
        for e in (a, b):
            e.fit_mask_run()
        J = len(fit_req)
        assert np.array_equal(a.fit_mask_rows(0, J), b.fit_mask_rows(0, J)) and np.array_equal(a.fit_counts(), b.fit_counts())

    def both(f):
        return [f(e) for e in (a, b)]

    fit_call(0, 1)
    res = a.read_residuals()
    batch, dom = DP.job_mix(res, labels, island, 0, level_size, parent, 2)
    out = both(lambda e: e.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                                batch.group_need, dom, 0, level_size, parent))
    assert np.array_equal(out[0][0], out[1][0]) and (out[0][1] == 0).any()
    fit_call(1, 3)
    donor = synth.make_inventory(3, 52, 0.5)
    upd = (np.array([5, 40, 700]), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # node 5 moves to rack 30, node 40 goes, node 700 joins rack 2
    both(lambda e: e.update_nodes(*upd))
    state["island"][[5, 40, 700]] = [30, -1, 2]
    state["labels"] = state["labels"].copy()
    state["labels"][[5, 40, 700]] = synth.island_labels(donor.labels, np.array([30, -1, 2], dtype=np.int32))
    fit_call(0, 4)
    both(lambda e: e.update_nodes(np.array([40]), np.array([PE_NODE_SET], dtype=np.uint8), np.ascontiguousarray(donor.cap.T[:1]),
                                  np.ascontiguousarray(donor.used.T[:1]), donor.labels[:1].copy(), np.array([1], dtype=np.int32)))
    state["island"][40] = 1
    state["labels"][40] = synth.island_labels(donor.labels[:1], np.array([1], dtype=np.int32))[0]
    fit_call(0, 5)                                         # the node that was added takes part
    both(lambda e: e.reset_residuals())
    fit_call(2, 6)
    # another hierarchy over the same inventory: nothing of the first one was kept
    state["sizes"], state["parent"] = [level_size[0], 3], (np.arange(level_size[0]) % 4 - 1).astype(np.int32)
    fit_call(1, 7)
    state["sizes"], state["parent"] = [level_size[0]], None
    fit_call(0, 8)
    # reload: another size, other islands
    island3, sizes3, parent3 = TC.tree("four", 700)
    inv3 = synth.make_inventory(700, 53)
    for e in (a, b):
        e.load_nodes(inv3.cap, inv3.used, inv3.labels, island3)
        e.jobs_upload(fit_req, fit_need)
    state.update(island=np.array(island3), labels=synth.island_labels(inv3.labels, island3), sizes=sizes3, parent=parent3)
    for level in range(4):
        fit_call(level, 9 + level)
    a.close()
    b.close()


def test_alternating_with_the_capacity_calls_and_the_placement():
    n = 1025
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 61)
    labels = synth.island_labels(inv.labels, island)
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    for e in (a, b):
        e.load_nodes(inv.cap, inv.used, inv.labels, island)
    req, need = synth.make_fit_jobs(40, 11)
    count = np.resize(np.array([1, 8, 40, 200, 1000], dtype=np.int32), 40)
    for step in range(3):
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, labels, island, step, level_size, parent, 90 + step)
        case = DP.Case(None, None, labels, island, level_size, parent, step, batch, dom)
        pj, pd = GF.pair_mix(case, step)
        GF.check_engine(a, case, pj, pd, load=False)
        for x, y in zip(a.gang_capacity(req, need), b.gang_capacity(req, need)):
            assert np.array_equal(x, y)
        GF.check_engine(a, case, pj, pd, load=False)
        for x, y in zip(a.gang_capacity_domains(req, need, count, level_size[0]),
                        b.gang_capacity_domains(req, need, count, level_size[0])):
            assert np.array_equal(x, y)
        GF.check_engine(a, case, pj, pd, load=False)
        for x, y in zip(a.gang_capacity_tree(req, need, count, None, level_size, parent),
                        b.gang_capacity_tree(req, need, count, None, level_size, parent)):
            assert np.array_equal(x, y)
        fits = GF.check_engine(a, case, pj, pd, load=False)[0]
        out = [e.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req, batch.group_need,
                                      dom, step, level_size, parent) for e in (a, b)]
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        assert np.array_equal(a.read_residuals(), b.read_residuals()) and a.stats()["pods_placed"] == b.stats()["pods_placed"]
        assert fits.any() and (out[0][1] == 0).any()
    a.close()
    b.close()


# ---------------------------------------------------------------- refusals

SENTINEL = 77


def raw(e, off, cnt, req, need, pj, pd, level, sizes, parent, outs, n_jobs=None, n_pairs=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(off, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32), arr(pj, np.int32),
            arr(pd, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    J = n_jobs if n_jobs is not None else len(keep[0]) - 1 if keep[0] is not None else 2
    P = n_pairs if n_pairs is not None else len(keep[4]) if keep[4] is not None else len(keep[5])
    L = len(keep[6]) if n_levels is None else n_levels
    rc = e.lib.pe_gang_fit_domains(e.h, J, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), P, ptr(keep[4]),
                                   ptr(keep[5]), level, L, ptr(keep[6]), ptr(keep[7]), *[ptr(o) for o in outs])
    return rc, e.lib.pe_last_error(e.h).decode()


def sentinels(P, J):
    return [np.full(P, SENTINEL, dtype=np.uint8), np.full(P, SENTINEL, dtype=np.int32), np.full(P, SENTINEL, dtype=np.int64),
            np.full(J, SENTINEL, dtype=np.int32)]


def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    off, cnt = [0, 1, 3], [2, 1, 3]
    req = np.array([Q, Q_GPU, Q], dtype=np.int64)
    need, pj, pd = [0, 1, 0], [1, 0, 1], [1, 2, 9]
    outs = sentinels(3, 2)
    good = dict(off=off, cnt=cnt, req=req, need=need, pj=pj, pd=pd, level=0, sizes=sizes, parent=parent)

    def refused(code, text, **change):
        rc, msg = raw(e, outs=outs, **dict(good, **change))
        assert rc == code and text in msg, (rc, msg, change)
        assert all((o == SENTINEL).all() for o in outs)

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before, stats = e.read_residuals(), e.stats()
    E = _abi.PE_EINVAL
    bad_req = req.copy()
    bad_req[1, 2] = -1
    # what pe_place_greedy_domains refuses about the groups
    refused(E, "negative request at index 6", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "job_group_off[0]", off=[1, 1, 3])
    refused(E, "not monotonic", off=[0, 2, 1])
    refused(E, "n_jobs < 0", n_jobs=-1)
    for name in ("off", "cnt", "req"):
        refused(E, "is NULL", **{name: None})
    # the pairs
    refused(E, "pair_job or pair_domain is NULL", pj=None)
    refused(E, "pair_job or pair_domain is NULL", pd=None)
    refused(E, "n_pairs outside", n_pairs=-1)
    refused(E, "n_pairs outside", n_pairs=2**31 - 1)
    refused(E, "pair_job: value outside [0, n_jobs) at index 1", pj=[1, 2, 0])
    refused(E, "pair_job: value outside [0, n_jobs) at index 0", pj=[-1, 2, 0])
    refused(E, "pair_job: value outside [0, n_jobs) at index 0", n_jobs=0, off=[0])
    refused(E, "pair_domain: value outside [0, level_size[level]) at index 2", pd=[1, 2, 10])
    refused(E, "pair_domain: value outside [0, level_size[level]) at index 1", pd=[1, -1, 10])
    refused(E, "at index 2", pd=[1, 2, 3], level=1)        # a leaf id that level 1 does not have
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
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    # the same arguments unchanged are accepted, and the sentinels go
    rc, msg = raw(e, outs=outs, **good)
    assert rc == _abi.PE_OK, msg
    assert all((o != SENTINEL).all() for o in outs)
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.gang_fit_domains(off, cnt, req, need, pj, pd, 7, sizes, parent)
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
        outs = sentinels(1, 1)
        rc, msg = raw(s, [0, 1], [2], np.array([Q], dtype=np.int64), [0], [0], [0], 0, sizes, parent, outs)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert all((o == SENTINEL).all() for o in outs) and np.array_equal(s.read_residuals(), before)
        s.close()
