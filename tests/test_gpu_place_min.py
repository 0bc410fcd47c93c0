"""pe_place_min_member_domains on the device against tests/min_member.py's checker (the C oracle, job by job):
every pod slot, every status, every group and job count and every residual cell, no sampling."""
import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import gang_fit as GF
import gang_ledger as GL
import min_member as MM
import tree_capacity as TC
from inventory_model import Model
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = MM.GiB
ISLAND = MM.ISLAND
Q, Q_GPU, ONE = MM.Q, MM.Q_GPU, MM.ONE
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working state is in LDS up to here


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def call(e, c, min_member="case"):
    b = c.batch
    mm = c.min_member if isinstance(min_member, str) else min_member
    return e.place_min_member_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, mm,
                                      c.job_domain, c.level, c.level_size, c.parent)


# ---------------------------------------------------------------- trees and sizes

@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 255, 257, 1025, 2500])
def test_trees(eng, name, n):
    for level in DP.tree_levels(name, n):
        c = MM.tree_case(name, n, level)
        _, st, gp, _ = MM.check_engine(eng, c)
        assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True)


@pytest.mark.parametrize("size", [1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 4097])
def test_domain_size(eng, size):
    c = MM.size_case(size)
    _, st, gp, _ = MM.check_engine(eng, c)
    assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True)
    assert st[2] == 1 and st[3] == 0 and gp[c.batch.job_group_off[4] + 1] == 3


def test_all_domains_active(eng):
    c = MM.all_active_case()
    _, st, gp, _ = MM.check_engine(eng, c)
    assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True)


@pytest.mark.parametrize("trap", sorted(MM.traps()))
def test_traps(eng, trap):
    c, want_st, want_gp = MM.traps()[trap]
    _, st, gp, _ = MM.check_engine(eng, c)
    assert st.tolist() == want_st and gp.tolist() == want_gp


# ---------------------------------------------------------------- counts

def test_100000_optional_zero_request_pods(eng):
    jobs = [(0, 9, 1, [(1, ONE, 0), (100000, [0, 0, 0, 0], 0)]),         # every optional pod at once, one node
            (0, 8, 2, [(100000, [0, 0, 0, 0], 1), (3, Q, 0)]),           # two mandatory, the rest in one decision
            (1, 5, 0, [(100000, Q, 0)])]                                 # as many as the five nodes hold
    c = MM.one_level_case([40, 5], jobs, seed=77)
    pods, st, gp, _ = MM.check_engine(eng, c)
    assert st.tolist() == [0, 0, 0] and gp[:3].tolist() == [1, 100000, 100000] and 0 < gp[4] < 100000
    assert len(set(pods[1:100001].tolist())) == 1


def test_optional_count_of_2_31_minus_1(eng):
    """One decision takes 2^31 - 1 zero-request pods; the checker cannot hold them, so the answer is stated outright."""
    big = 2**31 - 1
    c = MM.rack_case(0, [(0, 0, 1, [(1, MM.gpus(2), 0), (big, [0, 0, 0, 0], 0)])])
    eng.load_nodes(c.cap, c.used, c.labels, c.island)
    pods, st, gp, jp = call(eng, c)
    assert st.tolist() == [0] and gp.tolist() == [1, big] and jp.tolist() == [big + 1]
    assert len(pods) == big + 1 and pods[0] in (0, 1)
    node = int(pods[1])
    assert node in (0, 1) and np.count_nonzero(pods[1:] != node) == 0
    want = c.residual().copy()
    want[:, int(pods[0])] -= np.array(MM.gpus(2))
    assert np.array_equal(eng.read_residuals(), want)


# ---------------------------------------------------------------- identities on the device

@pytest.mark.parametrize("name", ["racks32", "four", "permuted"])
def test_min_member_all_is_place_greedy_domains(eng, name):
    n = 1025
    for level in DP.tree_levels(name, n):
        c = MM.tree_case(name, n, level)
        eng.load_nodes(c.cap, c.used, c.labels, c.island)
        b = c.batch
        pods, st = eng.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                            c.job_domain, c.level, c.level_size, c.parent)
        res = eng.read_residuals()
        assert (st == 0).any() and (st == 1).any()
        _, _, _, T = MM.shares(b, None)
        for mm in (None, np.full(len(T), -1, dtype=np.int32), np.array(T, dtype=np.int32)):
            eng.reset_residuals()
            p2, s2, gp, jp = call(eng, c, mm)
            assert np.array_equal(p2, pods) and np.array_equal(s2, st) and np.array_equal(eng.read_residuals(), res)
            assert jp.tolist() == [0 if s else t for s, t in zip(st.tolist(), T)]
            assert int(gp.sum()) == int(jp.sum())


@pytest.mark.parametrize("name", ["racks32", "four", "fanin"])
def test_min_member_zero_places_the_domains_slots(eng, name):
    n = 1025
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    eng.load_nodes(cap, used, labels, island)
    for q, nd in ((Q, 0), (Q_GPU, 1)):
        req, need = np.array([q], dtype=np.int64), np.array([nd], dtype=np.uint32)
        eng.reset_residuals()
        dc = eng.gang_capacity_domains(req, need, np.array([1], dtype=np.int32), level_size[0])
        row = dc.dom_slots[0]
        count = max(1, int(np.median(row)))
        batch, dom, mm = MM.make_batch([(d, 0, 0, [(count, q, nd)]) for d in range(level_size[0])])
        _, st, gp, jp = call(eng, MM.Case(cap, used, labels, island, list(level_size), parent, 0, batch, dom, mm))
        assert (st == 0).all() and gp.tolist() == np.minimum(row, count).tolist() and jp.tolist() == gp.tolist()
        assert (gp < count).any() and (gp == count).any()


@pytest.mark.parametrize("name,level", [("racks32", 0), ("racks32", 1), ("four", 2)])
def test_release_and_assume_of_the_outputs(eng, name, level):
    c = MM.tree_case(name, 1025, level)
    eng.load_nodes(c.cap, c.used, c.labels, c.island)
    before = eng.read_residuals()
    pods, st, gp, jp = call(eng, c)
    after = eng.read_residuals()
    assert (pods == -1).any() and (pods >= 0).any() and not np.array_equal(after, before)
    gangs = GL.of_batch(c.batch, pods)
    assert eng.release_gangs(*gangs.arrays()) == int(gp.sum()) == int(jp.sum())
    assert np.array_equal(eng.read_residuals(), before)
    eng.reset_residuals()
    assert eng.assume_gangs(*gangs.arrays()) == int(gp.sum())
    assert np.array_equal(eng.read_residuals(), after)


# ---------------------------------------------------------------- optional arguments

SENTINEL = -77


def raw(e, off, pri, cnt, req, need, mm, dom, level, sizes, parent, pods, st, gp, jp, n_jobs=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(off, np.int32), arr(pri, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32),
            arr(mm, np.int32), arr(dom, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    J = n_jobs if n_jobs is not None else len(keep[0]) - 1 if keep[0] is not None else len(keep[1])
    L = len(keep[7]) if n_levels is None else n_levels
    rc = e.lib.pe_place_min_member_domains(e.h, J, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                           ptr(keep[5]), ptr(keep[6]), level, L, ptr(keep[7]), ptr(keep[8]), ptr(pods),
                                           ptr(st), ptr(gp), ptr(jp))
    return rc, e.lib.pe_last_error(e.h).decode()


def test_each_output_null_in_turn_and_null_inputs(eng):
    c = MM.tree_case("racks32", 257, 0)
    b = c.batch
    eng.load_nodes(c.cap, c.used, c.labels, c.island)
    want = MM.place(eng.read_residuals(), c.labels, c.island, b, c.min_member, c.job_domain, 0, c.level_size, c.parent)
    J, G, P = len(b.priority), len(b.group_count), len(want[0])
    for skip in ("gp", "jp", "both", None):
        eng.reset_residuals()
        pods, st = np.full(P, SENTINEL, dtype=np.int32), np.full(J, SENTINEL, dtype=np.int32)
        gp, jp = np.full(G, SENTINEL, dtype=np.int32), np.full(J, SENTINEL, dtype=np.int64)
        rc, msg = raw(eng, b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, c.min_member, c.job_domain,
                      0, c.level_size, c.parent, pods, st, None if skip in ("gp", "both") else gp,
                      None if skip in ("jp", "both") else jp)
        assert rc == _abi.PE_OK, msg
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1]) and np.array_equal(eng.read_residuals(), want[3])
        assert (gp == SENTINEL).all() if skip in ("gp", "both") else np.array_equal(gp, want[2])
        assert (jp == SENTINEL).all() if skip in ("jp", "both") else jp.sum() == want[2].sum()
    # the two outputs that are not optional
    for no_pods, no_st, text in ((True, False, "out_pod_node is NULL"), (False, True, "out_job_status is NULL")):
        eng.reset_residuals()
        before = eng.read_residuals()
        pods, st = np.full(P, SENTINEL, dtype=np.int32), np.full(J, SENTINEL, dtype=np.int32)
        rc, msg = raw(eng, b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, c.min_member, c.job_domain,
                      0, c.level_size, c.parent, None if no_pods else pods, None if no_st else st, None, None)
        assert rc == _abi.PE_EINVAL and text in msg
        assert (pods == SENTINEL).all() and (st == SENTINEL).all() and np.array_equal(eng.read_residuals(), before)
    # group_need NULL = 0, min_member NULL = -1 everywhere
    for need, mm in ((None, c.min_member), (b.group_need, None), (None, None)):
        eng.reset_residuals()
        b0 = synth.JobBatch(b.job_group_off, b.priority, b.group_count, b.group_req,
                            np.zeros(G, dtype=np.uint32) if need is None else b.group_need, b.kind)
        w = MM.place(eng.read_residuals(), c.labels, c.island, b0, mm, c.job_domain, 0, c.level_size, c.parent)
        pods, st, gp, jp = eng.place_min_member_domains(b.job_group_off, b.priority, b.group_count, b.group_req, need, mm,
                                                        c.job_domain, 0, c.level_size, c.parent)
        assert np.array_equal(pods, w[0]) and np.array_equal(st, w[1]) and np.array_equal(gp, w[2])
        assert np.array_equal(eng.read_residuals(), w[3])


# ---------------------------------------------------------------- state

def test_state_across_calls():
    """The call, a node update, the call again, then a reset -- beside the model, with pe_stats' deltas."""
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

    def min_call(level, seed):
        batch, dom, mm = MM.job_mix(model.res, model.labels, model.island, level, level_size, parent, seed)
        want = MM.place(model.res, model.labels, model.island, batch, mm, dom, level, level_size, parent)
        s0 = e.stats()
        pods, st, gp, jp = e.place_min_member_domains(batch.job_group_off, batch.priority, batch.group_count,
                                                      batch.group_req, batch.group_need, mm, dom, level, level_size, parent)
        s1 = e.stats()
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1]) and np.array_equal(gp, want[2])
        assert MM.conditions(batch, mm, st, gp) == (True, True, True, True)
        model.res = want[3]
        want_stats = dict(s0)
        want_stats["jobs_placed"] += int((st == 0).sum())
        want_stats["jobs_failed"] += int((st == 1).sum())
        want_stats["pods_placed"] += int(want[2].sum())    # the pods that hold a node, not the placed jobs' totals
        assert s1 == want_stats                            # nothing else in pe_stats moves
        assert int(jp.sum()) == int(want[2].sum()) < int((pods >= -1).sum())
        same_state()

    same_state()
    min_call(0, 1)
    donor = synth.make_inventory(3, 52, 0.5)
    upd = (np.array([5, 40, 700]), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # node 5 moves to rack 30, node 40 goes, node 700 joins rack 2
    e.update_nodes(*upd)
    model.update(upd)
    same_state()
    min_call(0, 2)
    min_call(1, 3)                                         # without a reset, another level
    e.reset_residuals()
    model.reset()
    same_state()
    min_call(2, 4)
    e.close()


def test_alternating_with_place_greedy_domains_and_gang_fit_domains(eng):
    n = 1025
    island, level_size, parent = TC.tree("racks32", n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 61), island)
    eng.load_nodes(cap, used, labels, island)
    for step in range(3):
        level = step % len(level_size)
        res = eng.read_residuals()
        batch, dom, mm = MM.job_mix(res, labels, island, level, level_size, parent, 90 + step)
        c = MM.Case(cap, used, labels, island, list(level_size), parent, level, batch, dom, mm)
        # the read-only what-if of every job alone, before: it changes nothing
        pj = np.arange(len(dom), dtype=np.int32)
        fit = eng.gang_fit_domains(batch.job_group_off, batch.group_count, batch.group_req, batch.group_need, pj, dom, level,
                                   level_size, parent)
        w_fit = GF.answers(res, labels, island, batch, pj, dom, level, level_size, parent)
        assert np.array_equal(fit.fits, w_fit[0]) and np.array_equal(eng.read_residuals(), res)
        want = MM.check_engine(eng, c, load=False)
        # pe_place_greedy_domains on what the call left
        res2 = eng.read_residuals()
        b2, d2 = DP.job_mix(res2, labels, island, level, level_size, parent, 190 + step)
        w2 = DP.place(res2, labels, island, b2, d2, level, level_size, parent)
        pods, st = eng.place_greedy_domains(b2.job_group_off, b2.priority, b2.group_count, b2.group_req, b2.group_need, d2,
                                            level, level_size, parent)
        assert np.array_equal(pods, w2[0]) and np.array_equal(st, w2[1]) and np.array_equal(eng.read_residuals(), w2[2])
        assert (want[1] == 0).any()


# ---------------------------------------------------------------- refusals

def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    off, pri, cnt = [0, 1, 3], [0, 1], [2, 1, 3]
    req = np.array([Q, Q_GPU, Q], dtype=np.int64)
    need, dom, mm = [0, 1, 0], [1, 2], [1, 2]
    pods = np.full(6, SENTINEL, dtype=np.int32)
    st = np.full(2, SENTINEL, dtype=np.int32)
    gp = np.full(3, SENTINEL, dtype=np.int32)
    jp = np.full(2, SENTINEL, dtype=np.int64)
    good = dict(off=off, pri=pri, cnt=cnt, req=req, need=need, mm=mm, dom=dom, level=0, sizes=sizes, parent=parent)

    def refused(code, text, **change):
        args = dict(good, **change)
        extra = {k: args.pop(k) for k in ("n_jobs", "n_levels", "no_pods", "no_st") if k in args}
        rc, msg = raw(e, pods=None if extra.pop("no_pods", False) else pods, st=None if extra.pop("no_st", False) else st,
                      gp=gp, jp=jp, **args, **extra)
        assert rc == code and text in msg, (rc, msg, change)
        assert (pods == SENTINEL).all() and (st == SENTINEL).all() and (gp == SENTINEL).all() and (jp == SENTINEL).all()

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before = e.read_residuals()
    stats = e.stats()
    E = _abi.PE_EINVAL
    bad_req = req.copy()
    bad_req[1, 2] = -1
    # what pe_place_greedy_domains refuses
    refused(E, "negative request at index 6", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "job_group_off[0]", off=[1, 1, 3])
    refused(E, "not monotonic", off=[0, 2, 1])
    refused(E, "n_jobs < 0", n_jobs=-1)
    for name in ("off", "pri", "cnt", "req"):
        refused(E, "is NULL", **{name: None})
    refused(E, "out_pod_node is NULL", no_pods=True)
    refused(E, "out_job_status is NULL", no_st=True)
    refused(E, "job_domain is NULL", dom=None)
    refused(E, "job_domain: value outside [0, level_size[level]) at index 1", dom=[9, 10])
    refused(E, "job_domain: value outside [0, level_size[level]) at index 0", dom=[-1, 10])
    refused(E, "at index 0", dom=[3, 0], level=1)
    refused(E, "level outside", level=-1)
    refused(E, "level outside", level=3)
    refused(E, "n_levels outside", n_levels=0)
    refused(E, "n_levels outside", n_levels=5, sizes=sizes + [1, 1])
    refused(E, "level_size is NULL", sizes=None, n_levels=3)
    refused(E, "level_size: value outside [1, PE_MAX_DOMAINS] at index 1", sizes=[10, 0, 1])
    refused(E, "parent is NULL", parent=None)
    bad_parent = np.array(parent).copy()
    bad_parent[4] = 3
    refused(E, "parent: value outside [-1, size of the level above) at index 4", parent=bad_parent)
    # min_member: T = [2, 4]
    refused(E, "min_member: value below -1 at index 0", mm=[-2, 9])
    refused(E, "min_member: value below -1 at index 1", mm=[2, -5])
    refused(E, "min_member: value above the job's pod total at index 0", mm=[3, 4])
    refused(E, "min_member: value above the job's pod total at index 1", mm=[2, 5])
    refused(E, "job_domain: value outside", mm=[3, 4], dom=[1, 99])      # the siblings' checks come first
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    # the same arguments unchanged are accepted, at the bounds too, and the sentinels go
    for ok in (mm, [2, 4], [0, 0], [-1, -1]):
        e.reset_residuals()
        rc, msg = raw(e, pods=pods, st=st, gp=gp, jp=jp, **dict(good, mm=ok))
        assert rc == _abi.PE_OK, msg
        assert (st != SENTINEL).all() and (pods != SENTINEL).all() and (gp != SENTINEL).all() and (jp != SENTINEL).all()
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.place_min_member_domains(off, pri, cnt, req, need, [2, 7], dom, 0, sizes, parent)
    assert ei.value.code == E and "min_member" in str(ei.value)
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
        rc, msg = raw(s, [0, 1], [0], [2], np.array([Q], dtype=np.int64), [0], [1], [0], 0, sizes, parent, pods, st, None,
                      None)
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
    rc, msg = raw(eng, None, None, None, None, None, None, None, 1, sizes, parent, None, None, None, None, n_jobs=0)
    assert rc == _abi.PE_OK, msg
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    # jobs without pods: all placed, nothing moves
    pods, st, gp, jp = eng.place_min_member_domains([0, 0, 1], [0, 0], [0], np.array([Q], dtype=np.int64), None, [0, -1],
                                                    [0, 9], 0, sizes, parent)
    assert pods.shape == (0,) and st.tolist() == [0, 0] and gp.tolist() == [0] and jp.tolist() == [0, 0]
    assert np.array_equal(eng.read_residuals(), before)
