"""pe_place_first_fit_domains on the device against tests/first_fit.py's checker: every pod slot, status, job pair
and residual cell, no sampling; the traps; the two identities against the engine's own calls; one context walked
through its life; and every refusal."""
import os
import re

import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import first_fit as FF
import gang_fit as GF
import tree_capacity as TC
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
Q = [16000, 64 * GiB, 0, 0]
Q_GPU = [8000, 32 * GiB, 2, 50 * GiB]
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working state is in LDS up to here


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def call(e, case, pj, pd, **kw):
    b = case.batch
    return e.place_first_fit_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, pj, pd,
                                     case.level, case.level_size, case.parent, **kw)


# ---------------------------------------------------------------- trees and sizes

@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 2500])
def test_trees(eng, name, n):
    placed = failed = later = 0
    for level in DP.tree_levels(name, n):
        case, pj, pd = FF.pairs_case(name, n, level)
        _, status, pair, _ = FF.check_engine(eng, case, pj, pd, python=n <= 257)
        cand = FF.candidates(pj, len(status))
        placed += int((status == 0).sum())
        failed += int((status == 1).sum())
        later += sum(1 for j, p in enumerate(pair) if p >= 0 and p != cand[j][0])
    assert placed > 0 and failed > 0 and (later > 0 or n == 1)


# ---------------------------------------------------------------- both kernel instances in one call

@pytest.mark.parametrize("big", [1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 1025, 2049, 4097])
def test_overflow_between_a_large_domain_and_two_small_ones(eng, big):
    case, pj, pd = FF.overflow_case(big)
    _, status, pair, _ = FF.check_engine(eng, case, pj, pd, python=big <= 65)
    assert FF.overflow_conditions(pj, pd, pair) == (True, big > 1)      # out of the large domain, and back into it
    assert (status == 0).any() and (status == 1).any()


# ---------------------------------------------------------------- the traps

def test_trap_priority(eng):
    case, pj, pd = FF.trap_priority()
    pods, status, pair, _ = FF.check_engine(eng, case, pj, pd, python=True)
    w = FF.TRAP_PRIORITY_WANT
    assert pods.tolist() == w["pods"] and status.tolist() == w["status"] and pair.tolist() == w["pair"]


def test_trap_chain(eng):
    case, pj, pd = FF.trap_chain()
    pods, status, pair, _ = FF.check_engine(eng, case, pj, pd, python=True)
    w = FF.TRAP_CHAIN_WANT
    assert pods.tolist() == w["pods"] and status.tolist() == w["status"] and pair.tolist() == w["pair"]


def test_trap_repeat(eng):
    case, pj, pd = FF.trap_repeat()
    _, status, pair, res = FF.check_engine(eng, case, pj, pd, python=True)
    w = FF.TRAP_REPEAT_WANT
    assert status.tolist() == w["status"] and pair.tolist() == w["pair"] and res[2][:2].tolist() == [0, 0]


def test_trap_all_one_domain(eng):
    case, pj, pd = FF.trap_all_one_domain()
    _, status, _, _ = FF.check_engine(eng, case, pj, pd)
    assert (status == 0).any() and (status == 1).any()


def test_largest_level_with_200_jobs(eng):
    n = 3000
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 65536, n).astype(np.int32)
    ids[:600] = ids[0]                                   # one crowded leaf among the sparse ones
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 29), ids)
    jobs = [(0, int(rng.integers(0, 3)), [(1 + i % 5, Q, 0)] + ([(2, [500, GiB, 0, 0], 0)] if i % 3 == 0 else []))
            for i in range(200)]
    batch, _ = DP.make_batch(jobs)
    case = DP.Case(cap, used, labels, island, [65536], None, 0, batch, None)
    lists = [[int(ids[rng.integers(0, n)]), int(ids[0]), int(rng.integers(0, 65536))][:1 + j % 3] for j in range(200)]
    lists[7] = [0, 65535, int(ids[0])]
    pj = np.array([j for j, c in enumerate(lists) for _ in c], dtype=np.int32)
    pd = np.array([d for c in lists for d in c], dtype=np.int32)
    order = rng.permutation(len(pj))
    # shuffled positions, each job's own order kept: sort the positions a job received
    pos = {}
    for at, p in enumerate(order):
        pos.setdefault(int(pj[p]), []).append(at)
    spj, spd = np.empty_like(pj), np.empty_like(pd)
    for j, c in enumerate(lists):
        for at, d in zip(sorted(pos[j]), c):
            spj[at], spd[at] = j, d
    _, status, pair, _ = FF.check_engine(eng, case, spj, spd)
    cand = FF.candidates(spj, 200)
    assert (status == 0).any() and (status == 1).any()
    assert any(p >= 0 and p != cand[j][0] for j, p in enumerate(pair))


# ---------------------------------------------------------------- edge shapes

def test_edge_shapes(eng):
    case = DP.one_level_case([40, 7, 0], [], seed=77)                      # domain 2 has no node
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    res = case.residual()
    ok1 = (dom == 1) & (res >= 0).all(axis=0)
    one = int(np.minimum(res[0][ok1] // 500, res[1][ok1] // GiB).max())    # what domain 1's best node holds
    jobs = [(0, 3, []),                                                     # 0: no groups, in a pair
            (0, 3, []),                                                     # 1: no groups, in no pair
            (0, 2, [(0, Q, 0), (0, Q_GPU, ISLAND)]),                        # 2: zero-count groups only
            (0, 2, [(100000, [0, 0, 0, 0], 0)]),                            # 3: 100 000 zero-request pods
            (0, 2, [(one, [500, GiB, 0, 0], ISLAND)]),                      # 4: an island group one node holds
            (0, 1, [(2, Q, 0), (one + 1, [500, GiB, 0, 0], ISLAND)]),       # 5: ... one no node of domain 1 holds; domain 0 does
            (0, 1, [(3, Q, 0), (3, [2**62, 0, 0, 0], ISLAND)]),             # 6: 3 x 2^62 overflows int64
            (0, 0, [(2, Q, 0)]),                                            # 7: only the domain without nodes
            (0, 0, [(0, Q, 0)])]                                            # 8: ... where a job without pods is placed
    case.batch, _ = DP.make_batch(jobs)
    pj = np.array([0, 2, 3, 3, 4, 5, 5, 6, 6, 7, 8, 4], dtype=np.int32)
    pd = np.array([2, 2, 2, 1, 1, 1, 0, 1, 0, 2, 2, 0], dtype=np.int32)
    pods, status, pair, _ = FF.check_engine(eng, case, pj, pd)
    assert status.tolist() == [0, 1, 0, 0, 0, 0, 1, 1, 0]
    assert pair.tolist() == [0, -1, 1, 3, 4, 6, -1, -1, 10]
    assert len(pods) == 100000 + one + 2 + (one + 1) + 3 + 3 + 2 and (pods[:100000] >= 0).all()
    # each output alone: no pairs asked for; and no need array (the island groups become plain ones)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    got = call(eng, case, pj, pd, pairs=False)
    assert got[2] is None and np.array_equal(got[0], pods) and np.array_equal(got[1], status)
    b = case.batch
    zero = synth.JobBatch(b.job_group_off, b.priority, b.group_count, b.group_req, np.zeros_like(b.group_need), b.kind)
    want = FF.place_first_fit(res, case.labels, case.island, zero, pj, pd, 0, case.level_size, None)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    got = eng.place_first_fit_domains(b.job_group_off, b.priority, b.group_count, b.group_req, None, pj, pd, 0, case.level_size)
    assert all(np.array_equal(x, y) for x, y in zip(got, want[:3])) and np.array_equal(eng.read_residuals(), want[3])
    assert want[2][5] == 5 and pair[5] == 6                # plain pods spread over domain 1's nodes
    # a batch without a pod: out_pod_node may be NULL
    off, pri, cnt = np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    req, sizes = np.array([Q], dtype=np.int64), np.array(case.level_size, dtype=np.int32)
    one_pair, st, jp = np.zeros(1, dtype=np.int32), np.full(1, 77, dtype=np.int32), np.full(1, 77, dtype=np.int32)
    rc = eng.lib.pe_place_first_fit_domains(eng.h, 1, off.ctypes.data, pri.ctypes.data, cnt.ctypes.data, req.ctypes.data, None,
                                            1, one_pair.ctypes.data, one_pair.ctypes.data, 0, 1, sizes.ctypes.data, None,
                                            None, st.ctypes.data, jp.ctypes.data)
    assert rc == _abi.PE_OK and st.tolist() == [0] and jp.tolist() == [0]


def test_no_jobs_and_no_pairs(eng):
    case = DP.tree_case("racks32", 300, 0)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before, stats = eng.read_residuals(), eng.stats()
    none = np.zeros(0, dtype=np.int32)
    sizes = np.array(case.level_size, dtype=np.int32)
    par = np.ascontiguousarray(case.parent, dtype=np.int32)
    rc = eng.lib.pe_place_first_fit_domains(eng.h, 0, None, None, None, None, None, 0, None, None, 2, len(sizes),
                                            sizes.ctypes.data, par.ctypes.data, None, None, None)
    assert rc == _abi.PE_OK
    pods, st, pair = eng.place_first_fit_domains([0], [], [], np.zeros((0, 4), dtype=np.int64), None, none, none, 0,
                                                 case.level_size, case.parent)
    assert pods.shape == st.shape == pair.shape == (0,)
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    pods, st, pair = call(eng, case, none, none)               # jobs and no pairs: every job unschedulable
    J = len(case.batch.job_group_off) - 1
    assert st.tolist() == [1] * J and pair.tolist() == [-1] * J and (pods == -1).all() and len(pods) > 0
    assert np.array_equal(eng.read_residuals(), before)
    now = eng.stats()
    assert now["jobs_failed"] == stats["jobs_failed"] + J and now["jobs_placed"] == stats["jobs_placed"]
    assert now["pods_placed"] == stats["pods_placed"]


# ---------------------------------------------------------------- the two identities, against the engine's own calls

@pytest.mark.parametrize("name,level", [("racks32", 0), ("four", 1), ("permuted", 0), ("orphans", 1), ("racks32", 2)])
def test_identities(eng, name, level):
    case = DP.tree_case(name, 1025, level)
    b = case.batch
    J = len(b.job_group_off) - 1
    other = Engine(0)                                          # freshly loaded, never makes the new call
    other.load_nodes(case.cap, case.used, case.labels, case.island)
    # one pair per job = place_greedy_domains with that pair's domain
    order = np.random.default_rng(level).permutation(J).astype(np.int32)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    pods, st, pair = call(eng, case, order, case.job_domain[order])
    w_pods, w_st = other.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                              case.job_domain, level, case.level_size, case.parent)
    assert np.array_equal(pods, w_pods) and np.array_equal(st, w_st)
    assert np.array_equal(eng.read_residuals(), other.read_residuals())
    inv = np.empty(J, dtype=np.int32)
    inv[order] = np.arange(J, dtype=np.int32)
    assert np.array_equal(pair, np.where(st == 0, inv, -1)) and (st == 0).any() and (st == 1).any()
    # one job in the call = gang_fit_domains' first fit on the same residuals
    other.reset_residuals()
    pj, pd = GF.pair_mix(case, 5 + level)
    seen = set()
    for j in range(0, J, 2):
        one = FF.single_job(b, j)
        mine = pd[pj == j]
        zeros = np.zeros(len(mine), dtype=np.int32)
        first = other.gang_fit_domains(one.job_group_off, one.group_count, one.group_req, one.group_need, zeros, mine, level,
                                       case.level_size, case.parent, tables=False).first
        eng.reset_residuals()
        _, _, got = eng.place_first_fit_domains(one.job_group_off, one.priority, one.group_count, one.group_req,
                                                one.group_need, zeros, mine, level, case.level_size, case.parent)
        assert got.tolist() == first.tolist()
        seen.add(int(first[0]) >= 0)
    assert True in seen
    other.close()


# ---------------------------------------------------------------- one context through its life

def test_one_context_through_its_life():
    n = 1200
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 51)
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    fit_req, fit_need = synth.make_fit_jobs(64, 9)
    for e in (a, b):
        e.load_nodes(inv.cap, inv.used, inv.labels, island)
        e.jobs_upload(fit_req, fit_need)                   # staged before all of it
    state = {"island": np.array(island), "labels": synth.island_labels(inv.labels, island), "sizes": level_size, "parent": parent}
    def both(f):
        return [f(e) for e in (a, b)]

    def masks_agree():
        both(lambda e: e.fit_mask_run())
        J = len(fit_req)
        assert np.array_equal(a.fit_mask_rows(0, J), b.fit_mask_rows(0, J)) and np.array_equal(a.fit_counts(), b.fit_counts())

    def first_fit(level, seed):
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, state["labels"], state["island"], level, state["sizes"], state["parent"], seed)
        case = DP.Case(None, None, state["labels"], state["island"], list(state["sizes"]), state["parent"], level, batch, dom)
        case, pj, pd = FF.pair_lists(case, seed, res)
        stats = a.stats()                                  # only the three counters move
        want = FF.check_engine(a, case, pj, pd, load=False)
        bt = case.batch
        placed = want[1] == 0
        pods = sum(int(np.clip(bt.group_count[bt.job_group_off[j]:bt.job_group_off[j + 1]], 0, None).sum())
                   for j in np.nonzero(placed)[0])
        stats["pods_placed"] += pods
        stats["jobs_placed"] += int(placed.sum())
        stats["jobs_failed"] += int((~placed).sum())
        assert a.stats() == stats and placed.any() and not placed.all()

    masks_agree()
    first_fit(0, 1)
    res = a.read_residuals()
    batch, _ = DP.job_mix(res, state["labels"], state["island"], 0, level_size, parent, 2)
    pods, st = a.place_greedy(batch.job_group_off, batch.priority, batch.group_count, batch.group_req, batch.group_need)
    assert (st == 0).any()
    first_fit(1, 3)
    donor = synth.make_inventory(3, 52, 0.5)
    upd = (np.array([5, 40, 700]), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # node 5 moves to rack 30, node 40 goes, node 700 joins rack 2
    both(lambda e: e.update_nodes(*upd))
    state["island"][[5, 40, 700]] = [30, -1, 2]
    state["labels"] = state["labels"].copy()
    state["labels"][[5, 40, 700]] = synth.island_labels(donor.labels, np.array([30, -1, 2], dtype=np.int32))
    first_fit(0, 4)
    both(lambda e: e.update_nodes(np.array([40]), np.array([PE_NODE_SET], dtype=np.uint8), np.ascontiguousarray(donor.cap.T[:1]),
                                  np.ascontiguousarray(donor.used.T[:1]), donor.labels[:1].copy(), np.array([1], dtype=np.int32)))
    state["island"][40] = 1
    state["labels"][40] = synth.island_labels(donor.labels[:1], np.array([1], dtype=np.int32))[0]
    first_fit(0, 5)                                        # the node that was added takes part
    both(lambda e: e.reset_residuals())
    assert np.array_equal(a.read_residuals(), b.read_residuals())      # bit-equal to the engine that never made the call
    masks_agree()                                          # the staged fit batch is still valid
    first_fit(2, 6)
    # another hierarchy over the same inventory: nothing of the first one was kept
    state["sizes"], state["parent"] = [level_size[0], 3], (np.arange(level_size[0]) % 4 - 1).astype(np.int32)
    first_fit(1, 7)
    state["sizes"], state["parent"] = [level_size[0]], None
    first_fit(0, 8)
    both(lambda e: e.reset_residuals())
    assert np.array_equal(a.read_residuals(), b.read_residuals())
    # reload: another size, other islands
    island3, sizes3, parent3 = TC.tree("four", 700)
    inv3 = synth.make_inventory(700, 53)
    for e in (a, b):
        e.load_nodes(inv3.cap, inv3.used, inv3.labels, island3)
        e.jobs_upload(fit_req, fit_need)
    state.update(island=np.array(island3), labels=synth.island_labels(inv3.labels, island3), sizes=sizes3, parent=parent3)
    for level in range(4):
        first_fit(level, 9 + level)
    both(lambda e: e.reset_residuals())
    assert np.array_equal(a.read_residuals(), b.read_residuals())
    masks_agree()
    a.close()
    b.close()


def test_alternating_with_the_capacity_calls_and_the_what_if():
    n = 1025
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 61)
    labels = synth.island_labels(inv.labels, island)
    a, b = Engine(0), Engine(0)                            # b follows through place_greedy_domains on a's choices
    for e in (a, b):
        e.load_nodes(inv.cap, inv.used, inv.labels, island)
    req, need = synth.make_fit_jobs(40, 11)
    count = np.resize(np.array([1, 8, 40, 200, 1000], dtype=np.int32), 40)
    for step in range(3):
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, labels, island, step, level_size, parent, 90 + step)
        case = DP.Case(None, None, labels, island, level_size, parent, step, batch, dom)
        case, pj, pd = FF.pair_lists(case, step, res)
        bt = case.batch
        _, status, pair, after = FF.check_engine(a, case, pj, pd, load=False)
        # b places the placed jobs in the domains a chose for them: the same residuals
        chosen = np.where(pair >= 0, pd[np.clip(pair, 0, None)], 0).astype(np.int32)
        keep = np.nonzero(status == 0)[0]
        sub, sub_dom = DP.make_batch([(int(chosen[j]), int(bt.priority[j]), GF.job_groups(bt, int(j))) for j in keep])
        _, st = b.place_greedy_domains(sub.job_group_off, sub.priority, sub.group_count, sub.group_req, sub.group_need, sub_dom,
                                       step, level_size, parent)
        assert (st == 0).all() and np.array_equal(b.read_residuals(), after)
        for x, y in zip(a.gang_capacity(req, need), b.gang_capacity(req, need)):
            assert np.array_equal(x, y)
        for x, y in zip(a.gang_capacity_domains(req, need, count, level_size[0]),
                        b.gang_capacity_domains(req, need, count, level_size[0])):
            assert np.array_equal(x, y)
        for x, y in zip(a.gang_capacity_tree(req, need, count, None, level_size, parent),
                        b.gang_capacity_tree(req, need, count, None, level_size, parent)):
            assert np.array_equal(x, y)
        GF.check_engine(a, case, pj, pd, load=False)       # the what-if on the residuals the call left
        assert (status == 0).any() and (status == 1).any()
    a.close()
    b.close()


def test_rounds_stay_within_their_bound(eng):
    """PE_CAP_EVENTS=1 leaves "A=<active domains> rounds=<n> kernels_ms=<t>" in pe_last_error."""
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        for case, pj, pd in (FF.trap_chain(), FF.trap_all_one_domain(), FF.pairs_case("four", 1025, 1), FF.overflow_case(1017)):
            eng.load_nodes(case.cap, case.used, case.labels, case.island)
            call(eng, case, pj, pd)
            m = re.fullmatch(r"A=(\d+) rounds=(\d+) kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode())
            assert m, eng.lib.pe_last_error(eng.h)
            model = FF.rounds_model(case.residual(), case.labels, case.island, case.batch, pj, pd, case.level, case.level_size,
                                    case.parent)
            assert int(m.group(1)) == len(set(pd.tolist()))
            assert model[4] <= int(m.group(2)) <= len(pj) + 1
    finally:
        del os.environ["PE_CAP_EVENTS"]


# ---------------------------------------------------------------- refusals

SENTINEL = -7                          # no output holds it: pods and pairs are >= -1, statuses 0 or 1


def raw(e, off, pri, cnt, req, need, pj, pd, level, sizes, parent, outs, n_jobs=None, n_pairs=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(off, np.int32), arr(pri, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32),
            arr(pj, np.int32), arr(pd, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    J = n_jobs if n_jobs is not None else len(keep[0]) - 1 if keep[0] is not None else 2
    P = n_pairs if n_pairs is not None else len(keep[5]) if keep[5] is not None else len(keep[6])
    L = len(keep[7]) if n_levels is None else n_levels
    rc = e.lib.pe_place_first_fit_domains(e.h, J, *[ptr(k) for k in keep[:5]], P, ptr(keep[5]), ptr(keep[6]), level, L,
                                          ptr(keep[7]), ptr(keep[8]), *[ptr(o) for o in outs])
    return rc, e.lib.pe_last_error(e.h).decode()


def sentinels(pods, J):
    return [np.full(pods, SENTINEL, dtype=np.int32), np.full(J, SENTINEL, dtype=np.int32), np.full(J, SENTINEL, dtype=np.int32)]


def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    off, pri, cnt = [0, 1, 3], [0, 1], [2, 1, 3]
    req = np.array([Q, Q_GPU, Q], dtype=np.int64)
    need, pj, pd = [0, 1, 0], [1, 0, 1], [1, 2, 9]
    outs = sentinels(6, 2)
    good = dict(off=off, pri=pri, cnt=cnt, req=req, need=need, pj=pj, pd=pd, level=0, sizes=sizes, parent=parent)

    def refused(code, text, **change):
        o = change.pop("outs", outs)
        rc, msg = raw(e, outs=o, **dict(good, **change))
        assert rc == code and text in msg, (rc, msg, change)
        assert all((x == SENTINEL).all() for x in outs)

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before, stats = e.read_residuals(), e.stats()
    E = _abi.PE_EINVAL
    bad_req = req.copy()
    bad_req[1, 2] = -1
    # what pe_place_greedy_domains refuses about the batch
    refused(E, "negative request at index 6", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "job_group_off[0]", off=[1, 1, 3])
    refused(E, "not monotonic", off=[0, 2, 1])
    refused(E, "n_jobs < 0", n_jobs=-1)
    for name in ("off", "pri", "cnt", "req"):
        refused(E, "is NULL", **{name: None})
    refused(E, "out_job_status", outs=[outs[0], None, outs[2]])
    refused(E, "out_pod_node", outs=[None, outs[1], outs[2]])
    # what pe_gang_fit_domains refuses about the pairs
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
        e.place_first_fit_domains(off, pri, cnt, req, need, pj, pd, 7, sizes, parent)
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
        outs = sentinels(2, 1)
        rc, msg = raw(s, [0, 1], [0], [2], np.array([Q], dtype=np.int64), [0], [0], [0], 0, sizes, parent, outs)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert all((o == SENTINEL).all() for o in outs) and np.array_equal(s.read_residuals(), before)
        s.close()
