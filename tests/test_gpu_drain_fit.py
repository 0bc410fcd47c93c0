"""pe_drain_fit_domains on the device against tests/drain_fit.py's checker: every fits, moved, fail_slot and target
cell, no sampling; the existing calls' own verdict on a second engine; the move carried out; that the call changes
nothing; and every refusal."""
import numpy as np
import pytest

import domain_placement as DP
import drain_fit as DF
import tree_capacity as TC
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
Q = [2000, 4 * GiB, 0, 0]
Q_GPU = [8000, 32 * GiB, 1, 10 * GiB]
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
    return int(cap.sum())


def claimed(case, gangs, node, domain, gone=()):
    """A DrainCase whose book CLAIMS its pods: the residuals are the inventory's as loaded (that residents really
    hold what the book says is the caller's business, as for pe_gang_preempt_domains' victims)."""
    res = case.residual()
    for g in gone:
        res[:, g] = DF.NEVER
    return DF.DrainCase(case, res, DF.make_book(gangs), np.array(node, dtype=np.int32), np.array(domain, dtype=np.int32),
                        list(gone))


# ---------------------------------------------------------------- the traps, the trees

@pytest.mark.parametrize("trap", sorted(DF.traps()))
def test_traps(eng, trap):
    dc, expected = DF.traps()[trap]
    want = DF.check_engine(eng, dc, python=True)
    if expected is not None:
        assert [x.tolist() for x in want] == [list(x) for x in expected]


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 257, 1025, 2500])
def test_trees(eng, name, n):
    fitting = failing = foreign = 0
    for level in DP.tree_levels(name, n):
        dc = DF.tree_drain_case(name, n, level)
        fits, moved, _, _ = DF.check_engine(eng, dc, python=n <= 257)
        dom = DP.dom_level(dc.case.island, level, dc.case.level_size, dc.case.parent)
        fitting += int((fits & (moved > 0)).sum())
        failing += int((fits == 0).sum())
        foreign += int((dom[dc.cand_node] != dc.cand_domain).sum())
    assert n == 1 or (fitting > 0 and failing > 0 and foreign > 0)


def test_an_active_domain_without_nodes(eng):
    case = DP.one_level_case([40, 7, 0], [], seed=77)                      # domain 2 has no node
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    a, b = (int(x) for x in np.nonzero(dom == 0)[0][:2])
    dc = claimed(case, [[(Q, 0, [a, a])], [(Q, 0, [-1])]], [a, b], [2, 2])
    fits, moved, fail, target = DF.check_engine(eng, dc, python=True)
    assert (fits.tolist(), moved.tolist(), fail.tolist(), target.tolist()) == ([0, 1], [0, 0], [0, -1], [-1, -1, -1])


# ---------------------------------------------------------------- domain sizes across the workgroup and LDS bounds

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 1024, 1025, 4097]


@pytest.mark.parametrize("size", SIZES)
def test_domain_size(eng, size):
    """A large domain beside a small one.  The candidates sit at the first and the last place of the large domain and
    at places 63 / 64 and 255 / 256, by node id (the order of a segment's places is the gather's, so ids stand in for
    them; thread i mod 256 owns place i whatever the order).  The first candidate's run takes every slot the rest of
    the domain has and one more: it fails, and the candidates after it need those slots again -- a working copy that
    is not refreshed, or an exclusion that is not undone, shows."""
    case = DP.one_level_case([size, 5], [], seed=size)
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    large, small = np.nonzero(dom == 0)[0], np.nonzero(dom == 1)[0]
    at = sorted(set(k for k in (0, 62, 63, 64, 254, 255, 256, size - 2, size - 1) if 0 <= k < size))
    nodes = [int(large[k]) for k in at]
    first = nodes[0]
    s = slots_of(case.residual(), large[large != first], Q_BIG)
    gangs = [[(Q_BIG, 0, [first] * (s + 1))]]
    for n in nodes[1:]:
        gangs.append([(Q, 0, [n, int(small[0]), n]), (Q_GPU, 1, [n])])
    gangs.append([(Q, 0, [int(small[1])] * 2)])
    node = nodes + [int(small[1]), int(small[2])]
    domain = [0] * len(nodes) + [0, 1]                                     # the small domain's node into the large one
    fits, moved, fail, _ = DF.check_engine(eng, claimed(case, gangs, node, domain))
    assert (fits[0], moved[0], fail[0]) == (0, s, s)
    assert size <= 2 or fits[1:].any()


@pytest.mark.parametrize("k", [0, 1, 31, 32, 33, 65])
def test_candidates_per_domain(eng, k):
    """k candidates in one domain: none, one, a unit less one, a unit, a unit and one, two units and one."""
    case = DP.one_level_case([80, 9], [], seed=100 + k)
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    large, small = np.nonzero(dom == 0)[0], np.nonzero(dom == 1)[0]
    nodes = [int(x) for x in large[:k]] + [int(small[0])]
    gangs = [[(Q, 0, [n, n]), (Q_GPU, 1, [n] * (1 + i % 3))] for i, n in enumerate(nodes)]
    if k:
        gangs[k - 1].append((Q, DP.NO_LABEL, [nodes[k - 1]]))              # the domain's last candidate cannot move
    fits, _, _, _ = DF.check_engine(eng, claimed(case, gangs, nodes, [0] * k + [1]), python=True)
    assert k == 0 or not fits[k - 1]


# ---------------------------------------------------------------- what is asked for

def test_null_arguments(eng):
    dc = DF.tree_drain_case("racks32", 257, 0)
    want = DF.check_engine(eng, dc)
    off, cnt, req, need, pod, cn, cd = (np.ascontiguousarray(x) for x in dc.call_args()[:7])
    c = dc.case
    sizes, par = np.array(c.level_size, dtype=np.int32), np.ascontiguousarray(c.parent, dtype=np.int32)
    C, S = len(cn), len(pod)
    for which in range(4):
        outs = [np.full(C, 77, dtype=np.uint8), np.full(C, 77, dtype=np.int64), np.full(C, 77, dtype=np.int64),
                np.full(S, 77, dtype=np.int32)]
        ptrs = [o.ctypes.data if k == which else None for k, o in enumerate(outs)]
        rc = eng.lib.pe_drain_fit_domains(eng.h, len(off) - 1, off.ctypes.data, cnt.ctypes.data, req.ctypes.data,
                                          need.ctypes.data, pod.ctypes.data, C, cn.ctypes.data, cd.ctypes.data, 0, len(sizes),
                                          sizes.ctypes.data, par.ctypes.data, *ptrs)
        assert rc == 0 and np.array_equal(outs[which], want[which])
        assert all((o == 77).all() for k, o in enumerate(outs) if k != which)
    assert eng.drain_fit_domains(*dc.call_args(), fits=False, moved=False, fail_slot=False, target=False) == (None,) * 4
    # no need array: 0 for every group (the island runs become plain ones)
    plain = eng.drain_fit_domains(off, cnt, req, None, pod, cn, cd, 0, c.level_size, c.parent)
    zero = DF.Book(dc.book.off, dc.book.cnt, dc.book.req, np.zeros_like(dc.book.need), dc.book.pod)
    assert DF.same(plain, DF.drain_oracle(dc.res, c.labels, c.island, zero, cn, cd, 0, c.level_size, c.parent))


def test_no_candidates_and_no_gangs(eng):
    dc = DF.tree_drain_case("racks32", 257, 1)
    DF.load_engine(eng, dc)
    stats = eng.stats()
    none = np.zeros(0, dtype=np.int32)
    c = dc.case
    got = eng.drain_fit_domains(*dc.book.args(), none, none, 1, c.level_size, c.parent)
    assert got.fits.shape == got.moved.shape == got.fail_slot.shape == (0,) and (got.target == -1).all()
    assert len(got.target) == len(dc.book.pod)
    got = eng.drain_fit_domains([0], [], np.zeros((0, 4), dtype=np.int64), None, None, dc.cand_node, dc.cand_domain, 1,
                                c.level_size, c.parent)
    C = len(dc.cand_node)
    assert got.fits.tolist() == [1] * C and got.moved.tolist() == [0] * C and got.fail_slot.tolist() == [-1] * C
    assert got.target.shape == (0,)
    assert np.array_equal(eng.read_residuals(), dc.res) and eng.stats() == stats


# ---------------------------------------------------------------- the existing calls' own verdict, and the move

@pytest.mark.parametrize("name,level", [("racks32", 0), ("four", 1), ("orphans", 1)])
def test_identity_with_the_existing_calls(eng, name, level):
    """On a freshly loaded second engine per candidate: PE_NODE_REMOVE of n, then gang_fit_domains and
    place_greedy_domains of the runs as one job in the target domain give the same fits, pods and pod nodes."""
    dc = DF.tree_drain_case(name, 1025, level)
    got = DF.check_engine(eng, dc)
    c, book = dc.case, dc.book
    group_of = book.group_of_slot()
    other = Engine(0)
    live = [k for k, n in enumerate(dc.cand_node) if not DF.removed(dc.res, int(n)) and (book.pod == n).any()]
    assert len(live) >= 10
    seen = set()
    for k in live[:20]:
        n, d = int(dc.cand_node[k]), int(dc.cand_domain[k])
        DF.load_engine(other, dc)
        other.update_nodes([n], [PE_NODE_REMOVE])
        slots = np.nonzero(book.pod == n)[0]
        runs = DF.runs_of(book, slots, group_of)
        one, dom = DP.make_batch([(d, 0, [(len(sl), [int(x) for x in book.req[g]], int(book.need[g])) for g, sl in runs])])
        fit = other.gang_fit_domains(one.job_group_off, one.group_count, one.group_req, one.group_need, [0], [d], level,
                                     c.level_size, c.parent)
        assert (int(fit.fits[0]), int(fit.pods[0])) == (int(got[0][k]), int(got[1][k]))
        pods, st = other.place_greedy_domains(one.job_group_off, one.priority, one.group_count, one.group_req, one.group_need,
                                              dom, level, c.level_size, c.parent)
        assert int(st[0]) == 1 - int(got[0][k])
        assert np.array_equal(pods, got[3][slots])             # -1 in every slot of a job that is not placed
        seen.add(int(st[0]))
    assert seen == {0, 1}
    other.close()


def test_acting_on_the_answer():
    """The book really assumed onto one engine; a candidate that fits is moved with release_gangs and assume_gangs of
    the helper's arrays, and the residuals are the checker's; then the call is asked again."""
    dc = DF.tree_drain_case("racks32", 1025, 0)
    c, book = dc.case, dc.book
    e = Engine(0)
    e.load_nodes(c.cap, c.used, c.labels, c.island)
    assert e.assume_gangs(book.off, book.cnt, book.req, book.pod) == int((book.pod >= 0).sum())
    e.update_nodes(dc.gone, [PE_NODE_REMOVE] * len(dc.gone))
    assert np.array_equal(e.read_residuals(), dc.res)
    want = DF.check_engine(e, dc, load=False)
    res = dc.res
    moved_some = 0
    for k in np.nonzero(want[0] & (want[1] > 0))[0][:3]:
        n = int(dc.cand_node[k])
        ans = e.drain_fit_domains(*dc.call_args())             # asked again: the earlier move took slots
        if not ans.fits[k]:
            continue
        give, take = ans.move_of(book.pod, n)
        pods = int((book.pod == n).sum())
        assert e.release_gangs(book.off, book.cnt, book.req, give) == pods
        assert e.assume_gangs(book.off, book.cnt, book.req, take) == pods
        res = DF.residual_after_move(res, book, ans.target, n)
        assert np.array_equal(e.read_residuals(), res)
        assert (res[:, n] == c.residual()[:, n]).all()         # the node is empty again
        book = DF.Book(book.off, book.cnt, book.req, book.need, np.where(book.pod == n, ans.target, book.pod).astype(np.int32))
        dc = DF.DrainCase(c, res, book, dc.cand_node, dc.cand_domain, dc.gone)
        DF.check_engine(e, dc, load=False)                     # the book as it stands now
        moved_some += 1
    assert moved_some >= 1
    e.close()


# ---------------------------------------------------------------- read-only

def test_read_only_across_calls():
    n = 1200
    island, level_size, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 51)
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    fit_req, fit_need = synth.make_fit_jobs(64, 9)
    for e in (a, b):
        e.load_nodes(inv.cap, inv.used, inv.labels, island)
        e.jobs_upload(fit_req, fit_need)                   # staged before all of it
    state = {"island": np.array(island), "labels": synth.island_labels(inv.labels, island), "sizes": level_size,
             "parent": parent, "books": []}

    def both(f):
        return [f(e) for e in (a, b)]

    def place(level, seed):
        """A job mix placed on both engines; what was placed joins the book."""
        res = a.read_residuals()
        batch, dom = DP.job_mix(res, state["labels"], state["island"], level, state["sizes"], state["parent"], seed)
        out = both(lambda e: e.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                                    batch.group_need, dom, level, state["sizes"], state["parent"]))
        assert np.array_equal(out[0][0], out[1][0]) and (out[0][1] == 0).any()
        poff = DP.pod_offsets(batch.group_count)
        for j in np.nonzero(out[0][1] == 0)[0]:
            g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
            if poff[g1] > poff[g0]:
                state["books"].append([([int(x) for x in batch.group_req[g]], int(batch.group_need[g]),
                                        out[0][0][poff[g]:poff[g + 1]].tolist()) for g in range(g0, g1)])

    def drain_call(level, seed):
        res = a.read_residuals()
        book = DF.make_book(state["books"])
        case = DP.Case(None, None, state["labels"], state["island"], list(state["sizes"]), state["parent"], level, None, None)
        node, domain, _ = DF.candidates(case, book, res, seed)
        dc = DF.DrainCase(case, res, book, node, domain, [])
        stats = a.stats()
        fits = DF.check_engine(a, dc, load=False)[0]       # (the residuals bit-equal to those before the call)
        assert fits.any() and len(node) > 10
        assert a.stats() == stats and np.array_equal(b.read_residuals(), res)
        for e in (a, b):
            e.fit_mask_run()
        J = len(fit_req)
        assert np.array_equal(a.fit_mask_rows(0, J), b.fit_mask_rows(0, J)) and np.array_equal(a.fit_counts(), b.fit_counts())

    place(0, 1)
    drain_call(0, 2)
    place(1, 3)
    drain_call(1, 4)
    donor = synth.make_inventory(3, 52, 0.5)
    free = [int(x) for x in np.setdiff1d(np.arange(n), DF.make_book(state["books"]).pod)[:3]]   # nodes without pods
    upd = (np.array(free), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # one moves to rack 30, one goes, one joins rack 2
    both(lambda e: e.update_nodes(*upd))
    state["island"][free] = [30, -1, 2]
    state["labels"] = state["labels"].copy()
    state["labels"][free] = synth.island_labels(donor.labels, np.array([30, -1, 2], dtype=np.int32))
    drain_call(0, 5)
    drain_call(2, 6)
    both(lambda e: e.reset_residuals())                    # the placements are gone from the residuals; the book
    drain_call(1, 7)                                       # still claims them
    island3, sizes3, parent3 = TC.tree("four", 700)        # reload: another size, other islands
    inv3 = synth.make_inventory(700, 53)
    for e in (a, b):
        e.load_nodes(inv3.cap, inv3.used, inv3.labels, island3)
        e.jobs_upload(fit_req, fit_need)
    state.update(island=np.array(island3), labels=synth.island_labels(inv3.labels, island3), sizes=sizes3, parent=parent3,
                 books=[])
    place(0, 8)
    for level in range(4):
        drain_call(level, 9 + level)
    a.close()
    b.close()


# ---------------------------------------------------------------- refusals

SENTINEL = 77


def raw(e, off, cnt, req, need, pod, cn, cd, level, sizes, parent, outs, n_gangs=None, n_cands=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(off, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32), arr(pod, np.int32),
            arr(cn, np.int32), arr(cd, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    V = n_gangs if n_gangs is not None else len(keep[0]) - 1 if keep[0] is not None else 2
    C = n_cands if n_cands is not None else len(keep[5]) if keep[5] is not None else len(keep[6])
    L = len(keep[7]) if n_levels is None else n_levels
    rc = e.lib.pe_drain_fit_domains(e.h, V, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), C,
                                    ptr(keep[5]), ptr(keep[6]), level, L, ptr(keep[7]), ptr(keep[8]), *[ptr(o) for o in outs])
    return rc, e.lib.pe_last_error(e.h).decode()


def sentinels(C, S):
    return [np.full(C, SENTINEL, dtype=np.uint8), np.full(C, SENTINEL, dtype=np.int64), np.full(C, SENTINEL, dtype=np.int64),
            np.full(S, SENTINEL, dtype=np.int32)]


def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    off, cnt = [0, 1, 3], [2, 1, 3]
    req = np.array([Q, Q_GPU, Q], dtype=np.int64)
    need, pod, cn, cd = [0, 1, 0], [5, 5, 40, 5, -1, 40], [5, 40, 299], [1, 2, 9]
    outs = sentinels(3, 6)
    good = dict(off=off, cnt=cnt, req=req, need=need, pod=pod, cn=cn, cd=cd, level=0, sizes=sizes, parent=parent)

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
    # what pe_release_gangs refuses about the book
    refused(E, "group_req: negative value in group at index 1", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "gang_group_off: not rising from 0 at index 0", off=[1, 1, 3])
    refused(E, "gang_group_off: not rising from 0 at index 2", off=[0, 2, 1])
    refused(E, "n_gangs outside", n_gangs=-1)
    refused(E, "n_gangs outside", n_gangs=2**31)
    refused(E, "gang_group_off is NULL", off=None)
    refused(E, "group_count or group_req is NULL", cnt=None)
    refused(E, "group_count or group_req is NULL", req=None)
    refused(E, "pod_node is NULL", pod=None)
    refused(E, "pod_node: value outside [-1, n_total) at index 2", pod=[5, 5, 300, 5, -1, 40])
    refused(E, "pod_node: value outside [-1, n_total) at index 4", pod=[5, 5, 40, 5, -2, 40])
    # the candidates
    refused(E, "cand_node or cand_domain is NULL", cn=None)
    refused(E, "cand_node or cand_domain is NULL", cd=None)
    refused(E, "n_cands outside", n_cands=-1)
    refused(E, "n_cands outside", n_cands=2**31 - 1)
    refused(E, "cand_node: value outside [0, n_total) at index 2", cn=[5, 40, 300])
    refused(E, "cand_node: value outside [0, n_total) at index 0", cn=[-1, 40, 300])
    refused(E, "cand_node: a node named twice at index 2", cn=[5, 40, 5])
    refused(E, "cand_domain: value outside [0, level_size[level]) at index 2", cd=[1, 2, 10])
    refused(E, "cand_domain: value outside [0, level_size[level]) at index 1", cd=[1, -1, 10])
    refused(E, "at index 2", cd=[1, 2, 3], level=1)        # a leaf id that level 1 does not have
    # what pe_gang_fit_domains refuses about the hierarchy and level
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
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    # the same arguments unchanged are accepted, and the sentinels go
    rc, msg = raw(e, outs=outs, **good)
    assert rc == _abi.PE_OK, msg
    assert all((o != SENTINEL).all() for o in outs)
    want = DF.drain_oracle(before, synth.island_labels(inv.labels, island), island,
                           DF.Book(*(np.asarray(x) for x in (off, cnt, req, need, pod))), cn, cd, 0, sizes, parent)
    assert all(np.array_equal(x, y) for x, y in zip(outs, want))
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.drain_fit_domains(off, cnt, req, need, pod, cn, cd, 7, sizes, parent)
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
        outs = sentinels(1, 2)
        rc, msg = raw(s, [0, 1], [2], np.array([Q], dtype=np.int64), [0], [5, 5], [5], [0], 0, sizes, parent, outs)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert all((o == SENTINEL).all() for o in outs) and np.array_equal(s.read_residuals(), before)
        s.close()
