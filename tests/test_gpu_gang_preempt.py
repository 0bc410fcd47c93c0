"""pe_gang_preempt_domains on the device against tests/gang_preempt.py's checker: every prefix, victims, count and
best cell, no sampling; the engine's own fit call on the sets the answer names; and that the call changes nothing."""
import numpy as np
import pytest

import domain_placement as DP
import gang_fit as GF
import gang_preempt as GP
import tree_capacity as TC
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working copy is in LDS up to here
I64_MAX = 2**63 - 1


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- trees and sizes

@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_trees(eng, name, n):
    zero = more = back = none = 0
    for level in DP.tree_levels(name, n):
        prefix, _, count, _ = GP.check_engine(eng, GP.tree_pcase(name, n, level), python=n <= 257)
        zero += int((prefix == 0).sum())
        more += int((prefix >= 1).sum())
        back += int(((count >= 0) & (count < prefix)).sum())
        none += int((prefix == -1).sum())
    assert zero > 0 and (n == 1 or (more > 0 and back > 0 and none > 0))


@pytest.mark.parametrize("size", [1, 63, 64, 65, LDS - 1, LDS, LDS + 1, 1025, 2049])
def test_domain_size(eng, size):
    """A contested domain of `size` nodes beside a small one: both kernel instances and the PL_LDS_NODES edge."""
    pc = GP.one_level_pcase([size, 5], seed=size)
    prefix, _, _, _ = GP.check_engine(eng, pc)
    assert (prefix >= 1).any() and (prefix == 0).any()


@pytest.mark.parametrize("trap", sorted(GP.TRAPS))
def test_traps(eng, trap):
    pc, want = GP.TRAPS[trap]()
    got = GP.check_engine(eng, pc, python=True)
    assert [a.tolist() for a in got] == [list(w) for w in want]


# ---------------------------------------------------------------- input variants

def many_victims(n_vic):
    """One node with nothing free; n_vic victims of 1 GPU each; jobs of 1, 64 and 65 GPUs."""
    vics = [(v, [(GP.gpus(1), [0])]) for v in range(n_vic)]
    jobs = [(0, 9, [(1, GP.gpus(g, 1000, GiB), 0)]) for g in (1, 64, 65)]
    return GP._trap([[640000], [640 * GiB], [0], [0]], [0], 1, vics, jobs, [(j, 0, list(range(64))) for j in range(3)])


def test_lists_of_64_and_65(eng):
    pc = many_victims(66)
    prefix, mask, count, best = GP.check_engine(eng, pc)
    assert prefix.tolist() == [1, 64, -1] and count.tolist() == [1, 64, -1] and int(mask[1]) == 2**64 - 1
    pc.pair_vic_off = np.array([0, 64, 128, 193], dtype=np.int32)
    pc.pair_vic = np.concatenate([np.arange(64), np.arange(64), np.arange(65)]).astype(np.int32)
    with pytest.raises(PlacementError) as ei:
        eng.gang_preempt_domains(*pc.call_args())
    assert ei.value.code == _abi.PE_EINVAL and "PE_MAX_PAIR_VICTIMS" in str(ei.value) and "at index 2" in str(ei.value)


def test_victim_of_100000_zero_request_pods(eng):
    """100 000 pod slots of a zero request on one node are one release record that frees nothing; the victim behind it
    frees what the job needs."""
    pc = GP._trap([[64000, 64000], [64 * GiB] * 2, [0, 0], [0, 0]], [0, 0], 1,
                  [(0, [([0, 0, 0, 0], [1] * 100000), (GP.gpus(1), [-1, 0, -1])]), (1, [(GP.gpus(2), [1, -1, 1])])],
                  [(0, 9, [(1, GP.gpus(4, 1000, GiB), 0)]), (0, 9, [(1, GP.gpus(1, 1000, GiB), 0)])],
                  [(0, 0, [0, 1]), (1, 0, [0, 1])])
    prefix, mask, count, best = GP.check_engine(eng, pc)
    assert prefix.tolist() == [2, 1] and mask.tolist() == [0b10, 0b01] and best.tolist() == [0, 1]


def test_islands_empty_domain_jobs_without_groups_and_no_need(eng):
    """Island groups among the victims and the incoming groups, a domain without nodes, jobs without groups, and the
    call without a need array."""
    pc = GP._trap([[64000] * 3, [64 * GiB] * 3, [0, 8, 0], [0] * 3], [0, 0, 2], 4,
                  [(0, [(GP.gpus(2), [0, 0, 0, 0])]), (1, [(GP.gpus(3), [2, 2])])],        # an island group's pods: one node
                  [(0, 9, [(2, GP.gpus(4, 1000, GiB), ISLAND)]),                           # 8 GPUs on one node
                   (0, 9, [(2, GP.gpus(4, 1000, GiB), ISLAND), (1, GP.gpus(8, 0, 0), 0)]),
                   (0, 9, []),                                                             # no groups: placed anywhere
                   (0, 9, [(0, GP.gpus(4), 0)]),                                           # no pods
                   (0, 9, [(1, GP.gpus(6, 1000, GiB), 0)])],
                  [(0, 0, [0]), (1, 0, [0, 1]), (1, 0, [1, 0]), (2, 1, []), (2, 1, [1]), (3, 3, [0]), (4, 1, [0, 1]),
                   (4, 2, [0, 1]), (4, 2, [1, 0]), (0, 1, [0, 1])])
    prefix, mask, count, best = GP.check_engine(eng, pc, python=True)
    assert prefix.tolist() == [0, 1, 2, 0, 0, 0, -1, 2, 1, -1] and mask.tolist() == [0, 1, 2, 0, 0, 0, 0, 2, 1, 0]
    assert best.tolist() == [0, 1, 3, 5, 7]
    b, c = pc.case.batch, pc.case
    plain = eng.gang_preempt_domains(b.job_group_off, b.group_count, b.group_req, None, *pc.vic.arrays(), pc.pair_job,
                                     pc.pair_domain, pc.pair_vic_off, pc.pair_vic, 0, c.level_size, None)
    b.group_need[:] = 0
    for got, want in zip(plain, pc.answers()):
        assert np.array_equal(got, want)
    assert plain.prefix[0] == 0 and plain.prefix[2] == 2


def test_each_output_null_and_empty_calls(eng):
    pc = GP.tree_pcase("racks32", 257, 1)
    want = GP.check_engine(eng, pc)
    before, stats = eng.read_residuals(), eng.stats()
    args = pc.call_args()
    sel = eng.gang_preempt_domains(*args, tables=False)
    assert sel.prefix is None and np.array_equal(sel.best, want[3])
    tab = eng.gang_preempt_domains(*args, best=False)
    assert tab.best is None and all(np.array_equal(x, y) for x, y in zip(tab[:3], want[:3]))
    assert eng.gang_preempt_domains(*args, tables=False, best=False) == (None, None, None, None)
    keep = [np.ascontiguousarray(a, dtype=t) for a, t in zip(args[:12], [np.int32, np.int32, np.int64, np.uint32, np.int32, np.int32,
                                                                         np.int64, np.int32, np.int32, np.int32, np.int32, np.int32])]
    sizes = np.ascontiguousarray(pc.case.level_size, dtype=np.int32)
    parent = np.ascontiguousarray(pc.case.parent, dtype=np.int32)
    J, V, P = len(keep[0]) - 1, len(keep[4]) - 1, len(keep[8])
    ptr = lambda a: a.ctypes.data   # noqa: E731

    def call(outs, n_jobs=J, n_vic=V, n_pairs=P):
        rc = eng.lib.pe_gang_preempt_domains(eng.h, n_jobs, *[ptr(a) for a in keep[:4]], n_vic, *[ptr(a) for a in keep[4:8]],
                                             n_pairs, *[ptr(a) for a in keep[8:12]], 1, len(sizes), ptr(sizes), ptr(parent),
                                             *[None if o is None else ptr(o) for o in outs])
        assert rc == _abi.PE_OK, eng.lib.pe_last_error(eng.h)

    for k in range(4):                                      # each output alone, and each output NULL in turn
        for alone in (True, False):
            outs = [np.full(P, 77, dtype=np.int32), np.full(P, 77, dtype=np.uint64), np.full(P, 77, dtype=np.int32),
                    np.full(J, 77, dtype=np.int32)]
            given = [o if (i == k) == alone else None for i, o in enumerate(outs)]
            call(given)
            for i, o in enumerate(given):
                assert o is None or np.array_equal(o, want[i]), (k, alone, i)
    # no pairs: best is all -1 and nothing else is written; no jobs; no victims
    outs = [np.full(P, 77, dtype=np.int32), np.full(P, 77, dtype=np.uint64), np.full(P, 77, dtype=np.int32), np.full(J, 77, dtype=np.int32)]
    call(outs, n_pairs=0)
    assert (outs[3] == -1).all() and all((o == 77).all() for o in outs[:3])
    call(outs, n_jobs=0, n_pairs=0)
    rc = eng.lib.pe_gang_preempt_domains(eng.h, 0, None, None, None, None, 0, None, None, None, None, 0, None, None, None, None,
                                         0, len(sizes), ptr(sizes), ptr(parent), None, None, None, None)
    assert rc == _abi.PE_OK
    empty = np.zeros(P + 1, dtype=np.int32)
    got = eng.gang_preempt_domains(*args[:4], [0], [], np.zeros((0, 4), dtype=np.int64), None, pc.pair_job, pc.pair_domain, empty,
                                   [], 1, pc.case.level_size, pc.case.parent)
    fit = eng.gang_fit_domains(*args[:4], pc.pair_job, pc.pair_domain, 1, pc.case.level_size, pc.case.parent)
    assert np.array_equal(got.prefix, np.where(fit.fits == 1, 0, -1)) and np.array_equal(got.best, fit.first)
    assert not got.victims.any() and fit.fits.any() and not fit.fits.all()
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats


# ---------------------------------------------------------------- identities against the engine's own calls

@pytest.mark.parametrize("name,level", [("racks32", 0), ("four", 1), ("permuted", 0)])
def test_the_fit_call_agrees_on_the_released_sets(eng, name, level):
    """With empty lists the call is gang_fit_domains.  For a pair with an answer, a fresh engine loaded with the final
    set released fits the job there; with the first prefix - 1 victims released instead it does not."""
    pc = GP.tree_pcase(name, 257, level)
    c, b = pc.case, pc.case.batch
    eng.load_nodes(c.cap, c.used, c.labels, c.island)
    got = eng.gang_preempt_domains(*pc.call_args())
    empty = np.zeros(len(pc.pair_job) + 1, dtype=np.int32)
    args = pc.call_args()
    bare = eng.gang_preempt_domains(*args[:10], empty, [], *args[12:])
    fit = eng.gang_fit_domains(*args[:4], *args[8:10], *args[12:])
    assert np.array_equal(bare.prefix >= 0, fit.fits == 1) and np.array_equal(bare.best, fit.first)
    assert np.array_equal(got.prefix == 0, fit.fits == 1)
    other = Engine(0)
    sample = np.nonzero(got.prefix >= 1)[0][:12]
    assert len(sample) > 0
    for p in sample:
        j, d, k = int(pc.pair_job[p]), int(pc.pair_domain[p]), int(got.prefix[p])
        lst = pc.pair_vic[pc.pair_vic_off[p]:pc.pair_vic_off[p + 1]]
        for victims, fits in ((GP.final_set(pc.pair_vic_off, pc.pair_vic, p, got.victims[p]), 1), (lst[:k - 1].tolist(), 0)):
            other.load_nodes(c.cap, GP.used_without(c, pc.vic, victims, d), c.labels, c.island)
            one = other.gang_fit_domains(b.job_group_off, b.group_count, b.group_req, b.group_need, [j], [d], level,
                                         c.level_size, c.parent)
            assert int(one.fits[0]) == fits, (p, victims)
    other.close()


# ---------------------------------------------------------------- read-only across a context's life

def test_stateful_use_leaves_no_trace():
    n = 1200
    island, level_size, parent = TC.tree("racks32", n)
    base = DP.tree_case("racks32", n, 0)
    vic, res, held = GP.resident_victims(base)
    used = base.cap - res
    inv_labels = synth.make_inventory(n, 23).labels
    a, b = Engine(0), Engine(0)                            # b never makes the new call
    fit_req, fit_need = synth.make_fit_jobs(64, 9)
    for e in (a, b):
        e.load_nodes(base.cap, used, inv_labels, island)
        e.jobs_upload(fit_req, fit_need)                   # a staged fit batch before all of it
    state = {"island": np.array(island), "labels": base.labels.copy()}

    def same():
        counters = [{k: v for k, v in e.stats().items() if isinstance(v, int)} for e in (a, b)]   # (the rest are timings)
        assert np.array_equal(a.read_residuals(), b.read_residuals()) and counters[0] == counters[1]
        for e in (a, b):
            e.fit_mask_run()
        J = len(fit_req)
        assert np.array_equal(a.fit_mask_rows(0, J), b.fit_mask_rows(0, J)) and np.array_equal(a.fit_counts(), b.fit_counts())

    def the_call(level, seed):
        now = a.read_residuals()
        case = DP.Case(now, np.zeros_like(now), state["labels"], state["island"], list(level_size), parent, level, None, None)
        case.batch, case.job_domain = GP.incoming_mix(now, case, vic, held if level == 0 else {}, seed)
        pj, pd = GF.pair_mix(case, seed)
        pvo, pv = GP.pair_lists(case, vic, pj, pd, seed)
        pc = GP.PCase(case, vic, pj, pd, pvo, pv)
        stats = a.stats()
        prefix = GP.check_engine(a, pc, load=False)[0]
        assert ((prefix >= 1).any() or level > 0) and a.stats() == stats
        same()
        return case

    case = the_call(0, 1)
    bt = case.batch
    out = [e.place_greedy_domains(bt.job_group_off, bt.priority, bt.group_count, bt.group_req, bt.group_need, case.job_domain,
                                  0, level_size, parent) for e in (a, b)]
    assert np.array_equal(out[0][0], out[1][0]) and (out[0][1] == 0).any()
    the_call(1, 2)
    donor = synth.make_inventory(3, 52, 0.5)
    upd = (np.array([5, 40, 700]), np.array([PE_NODE_SET, PE_NODE_REMOVE, PE_NODE_SET], dtype=np.uint8),
           np.ascontiguousarray(donor.cap.T), np.ascontiguousarray(donor.used.T), donor.labels.copy(),
           np.array([30, -1, 2], dtype=np.int32))          # node 5 moves to rack 30, node 40 goes, node 700 joins rack 2
    for e in (a, b):
        e.update_nodes(*upd)
    state["island"][[5, 40, 700]] = [30, -1, 2]
    state["labels"][[5, 40, 700]] = synth.island_labels(donor.labels, np.array([30, -1, 2], dtype=np.int32))
    the_call(0, 3)                                         # victims' pods on the removed slot count nothing
    for e in (a, b):
        e.reset_residuals()
    same()                                                 # the reset snapshot is the one of an engine that never called
    the_call(2, 4)
    for e in (a, b):
        e.load_nodes(base.cap, used, inv_labels, island)
        e.jobs_upload(fit_req, fit_need)
    state.update(island=np.array(island), labels=base.labels.copy())
    the_call(0, 5)
    for e in (a, b):
        e.reset_residuals()
    same()
    a.close()
    b.close()


# ---------------------------------------------------------------- refusals

SENTINEL = 77
NAMES = ("off", "cnt", "req", "need", "voff", "vcnt", "vreq", "vpod", "pj", "pd", "pvo", "pv", "sizes", "parent")
TYPES = (np.int32, np.int32, np.int64, np.uint32, np.int32, np.int32, np.int64, np.int32, np.int32, np.int32, np.int32, np.int32,
         np.int32, np.int32)


def raw(e, outs, level=0, n_jobs=None, n_vic=None, n_pairs=None, n_levels=None, **arrays):
    keep = {k: None if arrays[k] is None else np.ascontiguousarray(arrays[k], dtype=t) for k, t in zip(NAMES, TYPES)}
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    J = n_jobs if n_jobs is not None else len(keep["off"]) - 1 if keep["off"] is not None else 2
    V = n_vic if n_vic is not None else len(keep["voff"]) - 1 if keep["voff"] is not None else 2
    P = n_pairs if n_pairs is not None else len(keep["pj"]) if keep["pj"] is not None else len(keep["pd"])
    L = len(keep["sizes"]) if n_levels is None else n_levels
    rc = e.lib.pe_gang_preempt_domains(e.h, J, *[ptr(keep[k]) for k in NAMES[:4]], V, *[ptr(keep[k]) for k in NAMES[4:8]], P,
                                       *[ptr(keep[k]) for k in NAMES[8:12]], level, L, ptr(keep["sizes"]), ptr(keep["parent"]),
                                       *[ptr(o) for o in outs])
    return rc, e.lib.pe_last_error(e.h).decode()


def sentinels(P, J):
    return [np.full(P, SENTINEL, dtype=np.int32), np.full(P, SENTINEL, dtype=np.uint64), np.full(P, SENTINEL, dtype=np.int32),
            np.full(J, SENTINEL, dtype=np.int32)]


def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    Q, Q_GPU = [16000, 64 * GiB, 0, 0], [8000, 32 * GiB, 2, 50 * GiB]
    good = dict(off=[0, 1, 3], cnt=[2, 1, 3], req=np.array([Q, Q_GPU, Q], dtype=np.int64), need=[0, 1, 0],
                voff=[0, 1, 3], vcnt=[2, 1, 2], vreq=np.array([Q, Q_GPU, Q], dtype=np.int64), vpod=[5, 6, 7, -1, 299],
                pj=[1, 0, 1], pd=[1, 2, 9], pvo=[0, 2, 2, 3], pv=[1, 0, 1], level=0, sizes=sizes, parent=parent)
    outs = sentinels(3, 2)

    def refused(code, text, **change):
        rc, msg = raw(e, outs, **dict(good, **change))
        assert rc == code and text in msg, (rc, msg, change)
        assert all((o == SENTINEL).all() for o in outs)

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before, stats = e.read_residuals(), e.stats()
    E = _abi.PE_EINVAL
    bad_req = good["req"].copy()
    bad_req[1, 2] = -1
    # everything pe_gang_fit_domains refuses: the groups, the pairs, the level, the hierarchy
    refused(E, "negative request at index 6", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "not monotonic", off=[0, 2, 1])
    refused(E, "n_jobs < 0", n_jobs=-1)
    for name in ("off", "cnt", "req"):
        refused(E, "is NULL", **{name: None})
    refused(E, "pair_job or pair_domain is NULL", pj=None)
    refused(E, "pair_job or pair_domain is NULL", pd=None)
    refused(E, "n_pairs outside", n_pairs=-1)
    refused(E, "pair_job: value outside [0, n_jobs) at index 1", pj=[1, 2, 0])
    refused(E, "pair_domain: value outside [0, level_size[level]) at index 2", pd=[1, 2, 10])
    refused(E, "level outside", level=3)
    refused(E, "n_levels outside", n_levels=0)
    refused(E, "level_size is NULL", sizes=None, n_levels=3)
    refused(E, "level_size: value outside [1, PE_MAX_DOMAINS] at index 1", sizes=[10, 0, 1])
    refused(E, "parent is NULL", parent=None)
    bad_parent = np.array(parent).copy()
    bad_parent[4] = 3
    refused(E, "parent: value outside [-1, size of the level above) at index 4", parent=bad_parent)
    # the victims
    refused(E, "n_victims outside", n_vic=-1)
    refused(E, "vic_group_off is NULL", voff=None)
    refused(E, "vic_group_off: not rising from 0 at index 0", voff=[1, 1, 3])
    refused(E, "vic_group_off: not rising from 0 at index 2", voff=[0, 3, 2])
    refused(E, "vic_group_count or vic_group_req is NULL", vcnt=None)
    refused(E, "vic_group_count or vic_group_req is NULL", vreq=None)
    refused(E, "vic_group_count: negative value at index 2", vcnt=[2, 1, -2])
    refused(E, "vic_group_req: negative value in group at index 1", vreq=bad_req)
    refused(E, "vic_pod_node is NULL", vpod=None)
    refused(E, "vic_pod_node: value outside [-1, n_total) at index 4", vpod=[5, 6, 7, -1, 300])
    refused(E, "vic_pod_node: value outside [-1, n_total) at index 1", vpod=[5, -2, 7, -1, 300])
    # the lists
    refused(E, "pair_vic_off is NULL", pvo=None)
    refused(E, "pair_vic_off: not rising from 0 at index 0", pvo=[1, 2, 2, 3])
    refused(E, "pair_vic_off: not rising from 0 at index 2", pvo=[0, 2, 1, 3])
    refused(E, "pair_vic is NULL", pv=None)
    refused(E, "pair_vic: value outside [0, n_victims) at index 2", pv=[1, 0, 2])
    refused(E, "pair_vic: value outside [0, n_victims) at index 0", pv=[-1, 0, 2])
    refused(E, "pair_vic: the same victim twice in one list at index 1", pv=[1, 1, 1])
    refused(E, "PE_MAX_PAIR_VICTIMS candidate victims for the pair at index 1", pvo=[0, 2, 67, 68], pv=[1, 0] + [0] * 66,
            voff=[0, 1, 3])
    # overflow: the residual plus ALL the call's victim pods on the node, listed in a pair or not
    assert before[1][7] >= 0
    big = np.array([Q, [0, I64_MAX - int(before[1][7]), 0, 0], Q], dtype=np.int64)
    rc, msg = raw(e, outs, **dict(good, vreq=big))          # exactly INT64_MAX on node 7: accepted
    assert rc == _abi.PE_OK, msg
    outs = sentinels(3, 2)
    big[1, 1] += 1
    refused(E, "overflow", vreq=big)
    refused(E, "at node 7", vreq=big, pvo=[0, 0, 0, 0], pv=[])
    big[0] = big[1] = [0, 2**62, 0, 0]
    refused(E, "at node 7", vreq=big, vpod=[7, -1, 7, -1, 299])                            # two records add up past int64
    refused(E, "at node 7", vreq=big, vcnt=[2, 2, 1], vpod=[5, 6, 7, 7, 299])              # a run's product
    big[1] = [2**62, 0, 0, 0]
    refused(E, "at node 9", vreq=big, vcnt=[0, 100000, 0], vpod=[9] * 100000)
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    # a removed slot takes no part in the guard
    e.update_nodes(np.array([7]), np.array([PE_NODE_REMOVE], dtype=np.uint8), None, None, None, None)
    rc, msg = raw(e, outs, **dict(good, vreq=big, vcnt=[1, 2, 2], vpod=[5, 7, 7, 6, 299]))
    assert rc == _abi.PE_OK, msg
    assert all((o != SENTINEL).all() for o in outs)
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.gang_preempt_domains(good["off"], good["cnt"], good["req"], good["need"], good["voff"], good["vcnt"], good["vreq"],
                               good["vpod"], good["pj"], good["pd"], good["pvo"], good["pv"], 7, sizes, parent)
    assert ei.value.code == E and "level" in str(ei.value)
    e.close()


def test_sharded_context_is_refused():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)
    inv = synth.make_inventory(n, 71)
    Q = [16000, 64 * GiB, 0, 0]
    for r in range(2):
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(inv.cap, inv.used, inv.labels, island)
        before = s.read_residuals()
        outs = sentinels(1, 1)
        rc, msg = raw(s, outs, off=[0, 1], cnt=[2], req=np.array([Q], dtype=np.int64), need=[0], voff=[0, 1], vcnt=[1],
                      vreq=np.array([Q], dtype=np.int64), vpod=[3], pj=[0], pd=[0], pvo=[0, 1], pv=[0], sizes=sizes, parent=parent)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert all((o == SENTINEL).all() for o in outs) and np.array_equal(s.read_residuals(), before)
        s.close()
