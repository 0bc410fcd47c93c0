"""pe_scale_up_domains on the device against tests/scale_up.py's checker: every nodes, fail_group, pods, new_pods and
best cell, no sampling; the existing calls' own verdict on a second engine after PE_NODE_SET of the template; that
the call changes nothing; the calls that share its buffers in turn; and every refusal."""
import numpy as np
import pytest

import domain_placement as DP
import drain_fit as DF
import gang_fit as GF
import scale_up as SU
import tree_capacity as TC
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the working copy is in LDS up to here


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- the traps, the trees

@pytest.mark.parametrize("trap", sorted(SU.traps()))
def test_traps(eng, trap):
    sc, expected = SU.traps()[trap]
    want = SU.check_engine(eng, sc, python=True)
    for got, exp, what in zip(want, expected, SU.NAMES):
        if exp is not None:
            assert got.tolist() == list(exp), what


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [257, 1025])
def test_trees(eng, name, n):
    for level in DP.tree_levels(name, n):
        nodes, _, _, new_pods, _ = SU.check_engine(eng, SU.tree_scale_case(name, n, level), python=n <= 257)
        assert (nodes == 0).any() and (nodes >= 2).any() and (nodes == -1).any() and (new_pods > 0).any()


# ---------------------------------------------------------------- domain sizes, K values, slot ids

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, LDS - 1, LDS, LDS + 1, 4097]


@pytest.mark.parametrize("K,sizes", [(0, SIZES), (1, SIZES), (2, SIZES), (63, [0, 64, LDS, 4097]), (64, [0, 1, 257, LDS + 1, 4097])])
def test_domain_sizes_and_new_nodes(eng, K, sizes):
    """Segments on both sides of the wave, the workgroup and the LDS bound (the new places are in registers: the LDS
    bound is the segment's alone) with K new nodes allowed, the new slots' ids scattered below, between and above
    every segment's.  Job 0 needs exactly K template nodes whatever the domain holds; job 1 mixes real and new."""
    sc = SU.sized_case(sizes, K, seed=500 + K, pairs_per_domain=3)
    nodes, _, _, new_pods, _ = SU.check_engine(eng, sc)
    first = sc.pair_job == 0
    assert (nodes[first] == (K if K else -1)).all() and (new_pods[first] == K).all()
    live = np.nonzero((sc.res[0] != SU.NEVER) & (np.asarray(sc.case.island) >= 0))[0]
    assert K == 0 or ((sc.new_slot < live.max()).any() and (sc.new_slot > live.min()).any())


def test_new_slots_below_and_above_every_id(eng):
    """The same rack with the new slots once all below and once all above the live ids: ties go the other way."""
    free = [SU.node(8)] * 3
    jobs = [[(2, SU.gpus(3), 0), (3, SU.gpus(5), 0)]]
    below = SU.make_case([None, None] + free, 0, jobs, [SU.node(8)], [0, 1], [(0, 0, 0, None)])
    above = SU.make_case(free, 2, jobs, [SU.node(8)], [3, 4], [(0, 0, 0, None)])
    a = SU.check_engine(eng, below, python=True)
    b = SU.check_engine(eng, above, python=True)
    assert a[0].tolist() == b[0].tolist() == [1] and a[3].tolist() != b[3].tolist()


@pytest.mark.parametrize("k", [1, 31, 32, 33, 65])
def test_pairs_per_domain(eng, k):
    """k pairs of one domain with unequal pair_max, so that a unit mixes attempt counts: a new place or a working
    copy left over from one pair to the next shows."""
    sc = SU.sized_case([80, 9], 4, seed=600 + k, pairs_per_domain=k)
    nodes, _, _, _, _ = SU.check_engine(eng, sc, python=True)
    assert len(nodes) == 2 * k and (k < 31 or len(set(sc.pair_max.tolist())) >= 4)
    assert (nodes > 0).any() or k == 1


# ---------------------------------------------------------------- what is asked for

def raw(e, jgo, cnt, req, need, tres, tlab, slot, pj, pd, pt, pm, level, sizes, parent, outs, n_jobs=None, n_templates=None,
        n_new=None, n_pairs=None, n_levels=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [arr(jgo, np.int32), arr(cnt, np.int32), arr(req, np.int64), arr(need, np.uint32), arr(tres, np.int64),
            arr(tlab, np.uint32), arr(slot, np.int32), arr(pj, np.int32), arr(pd, np.int32), arr(pt, np.int32),
            arr(pm, np.int32), arr(sizes, np.int32), arr(parent, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    J = n_jobs if n_jobs is not None else len(keep[0]) - 1
    T = n_templates if n_templates is not None else len(keep[4].reshape(-1, 4)) if keep[4] is not None else 1
    N = n_new if n_new is not None else len(keep[6]) if keep[6] is not None else 1
    P = n_pairs if n_pairs is not None else max(len(x) for x in keep[7:10] if x is not None)
    L = len(keep[11]) if n_levels is None else n_levels
    rc = e.lib.pe_scale_up_domains(e.h, J, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), T, ptr(keep[4]),
                                   ptr(keep[5]), N, ptr(keep[6]), P, ptr(keep[7]), ptr(keep[8]), ptr(keep[9]), ptr(keep[10]),
                                   level, L, ptr(keep[11]), ptr(keep[12]), *[ptr(o) for o in outs])
    return rc, e.lib.pe_last_error(e.h).decode()


SENTINEL = 77


def sentinels(P, J):
    return [np.full(P, SENTINEL, dtype=np.int32), np.full(P, SENTINEL, dtype=np.int32), np.full(P, SENTINEL, dtype=np.int64),
            np.full(P, SENTINEL, dtype=np.int64), np.full(J, SENTINEL, dtype=np.int32)]


def test_null_arguments(eng):
    sc = SU.tree_scale_case("racks32", 257, 0)
    want = SU.check_engine(eng, sc)
    args = sc.call_args()
    P, J = len(sc.pair_job), len(sc.case.batch.job_group_off) - 1
    for which in range(5):                                  # each output alone
        outs = sentinels(P, J)
        rc, msg = raw(eng, *args, [o if k == which else None for k, o in enumerate(outs)])
        assert rc == 0, msg
        assert np.array_equal(outs[which], want[which])
        assert all((o == SENTINEL).all() for k, o in enumerate(outs) if k != which)
    for which in range(5):                                  # each output left out in turn
        outs = sentinels(P, J)
        rc, msg = raw(eng, *args, [None if k == which else o for k, o in enumerate(outs)])
        assert rc == 0, msg
        assert all(np.array_equal(o, w) for k, (o, w) in enumerate(zip(outs, want)) if k != which)
        assert (outs[which] == SENTINEL).all()
    assert eng.scale_up_domains(*args, nodes=False, fail_group=False, pods=False, new_pods=False, best=False) == (None,) * 5
    c = sc.case
    zero_need = DP.Case(c.cap, c.used, c.labels, c.island, c.level_size, c.parent, c.level,
                        synth.JobBatch(c.batch.job_group_off, c.batch.priority, c.batch.group_count, c.batch.group_req,
                                       np.zeros_like(c.batch.group_need), c.batch.kind), c.job_domain)
    variants = [SU.ScaleCase(zero_need, sc.res, sc.gone, *args[4:11]),                           # group_need NULL = 0
                SU.ScaleCase(c, sc.res, sc.gone, sc.tmpl_res, None, *args[6:11]),                # tmpl_labels NULL = 0
                SU.ScaleCase(c, sc.res, sc.gone, *args[4:10], None)]                             # pair_max NULL = n_new
    for k, v in enumerate(variants):
        a = list(v.call_args())
        if k == 0:
            a[3] = None
        got = eng.scale_up_domains(*a)
        assert SU.same(got, SU.scale_oracle(v)), k
        assert not SU.same(got, want), k                   # the argument mattered


def test_no_pairs_and_no_jobs(eng):
    sc = SU.tree_scale_case("racks32", 257, 1)
    SU.load_engine(eng, sc)
    stats = eng.stats()
    none = np.zeros(0, dtype=np.int32)
    a = list(sc.call_args())
    a[7:11] = [none, none, none, none]
    got = eng.scale_up_domains(*a)
    assert got.nodes.shape == got.fail_group.shape == got.pods.shape == got.new_pods.shape == (0,)
    assert (got.best == -1).all() and len(got.best) == len(sc.case.batch.job_group_off) - 1
    got = eng.scale_up_domains([0], [], np.zeros((0, 4), dtype=np.int64), None, np.zeros((0, 4), dtype=np.int64), None, none,
                               none, none, none, None, 1, sc.case.level_size, sc.case.parent)
    assert got.best.shape == (0,) and got.nodes.shape == (0,)
    assert np.array_equal(eng.read_residuals(), sc.res) and eng.stats() == stats


# ---------------------------------------------------------------- the existing calls' own verdict

def leaf_under(case, d):
    """A leaf whose level-`level` domain is d, or None."""
    leaves = np.arange(int(case.level_size[0]), dtype=np.int32)
    dom = DP.dom_level(leaves, case.level, case.level_size, case.parent)
    at = np.nonzero(dom == d)[0]
    return int(at[0]) if len(at) else None


def identity(eng, sc, limit):
    """On a second engine per pair: PE_NODE_SET of the template on new_slot[0 .. k) under a leaf of the domain, one
    node at a time; gang_fit_domains says 0 for every k < out_nodes and 1 at out_nodes (0 up to pair_max where the
    answer is -1), and place_greedy_domains of the job alone then places it with out_new_pods pods on the new slots."""
    got = SU.check_engine(eng, sc)
    c, b = sc.case, sc.case.batch
    other = Engine(0)
    seen, done = set(), 0
    for p in np.argsort(-got[0], kind="stable"):           # the pairs with the most new nodes first
        j, d, t, K = int(sc.pair_job[p]), int(sc.pair_domain[p]), int(sc.pair_template[p]), int(sc.kmax()[p])
        leaf = leaf_under(c, d)
        if leaf is None or (j, d, t, K) in seen or done >= limit:
            continue
        seen.add((j, d, t, K))
        done += 1
        SU.load_engine(other, sc)
        g0, g1 = int(b.job_group_off[j]), int(b.job_group_off[j + 1])
        one = ([0, g1 - g0], b.group_count[g0:g1], b.group_req[g0:g1], b.group_need[g0:g1])
        last = int(got[0][p]) if got[0][p] >= 0 else K
        for k in range(last + 1):
            if k > 0:
                lab = 0 if sc.tmpl_labels is None else int(sc.tmpl_labels[t])
                other.update_nodes([int(sc.new_slot[k - 1])], [PE_NODE_SET], sc.tmpl_res[t].reshape(1, 4),
                                   np.zeros((1, 4), dtype=np.int64), [lab], [leaf])
            fit = other.gang_fit_domains(*one, [0], [d], c.level, c.level_size, c.parent)
            assert int(fit.fits[0]) == int(k == got[0][p]), (p, k)
        assert (int(fit.fail_group[0]), int(fit.pods[0])) == (int(got[1][p]), int(got[2][p]))
        if got[0][p] >= 0:
            pods, st = other.place_greedy_domains(one[0], [0], *one[1:], [d], c.level, c.level_size, c.parent)
            assert int(st[0]) == 0
            assert int(np.isin(pods, sc.new_slot[:last]).sum()) == int(got[3][p])
    other.close()
    return done


@pytest.mark.parametrize("trap", ["worked", "non_monotone_issue", "non_monotone_from_zero", "tie_new_below", "tie_new_above",
                                  "island_on_new", "need_on_template", "island_bit_set", "empty_domain", "best_not_first"])
def test_identity_on_traps(eng, trap):
    assert identity(eng, SU.traps()[trap][0], 4) >= 1


@pytest.mark.parametrize("name,level", [("racks32", 0), ("four", 1), ("orphans", 1)])
def test_identity_with_the_existing_calls(eng, name, level):
    assert identity(eng, SU.tree_scale_case(name, 257, level), 8) >= 6


# ---------------------------------------------------------------- read-only, and the shared buffers

def test_read_only_across_calls():
    """A walk beside an engine that never makes the call: residuals, the fit mask rows of a staged batch and the
    stats stay bit-equal through placements, node updates, a reset and a reload."""
    a, b = Engine(0), Engine(0)
    fit_req, fit_need = synth.make_fit_jobs(64, 9)

    def both(f):
        return [f(e) for e in (a, b)]

    def scale_call(sc):
        res, stats = a.read_residuals(), a.stats()
        now = SU.ScaleCase(sc.case, res, sc.gone, *sc.call_args()[4:11])
        nodes = SU.check_engine(a, now, load=False)[0]     # (the residuals bit-equal to those before the call)
        assert (nodes > 0).any()
        assert a.stats() == stats and np.array_equal(b.read_residuals(), res)
        both(lambda e: e.fit_mask_run())
        J = len(fit_req)
        assert np.array_equal(a.fit_mask_rows(0, J), b.fit_mask_rows(0, J)) and np.array_equal(a.fit_counts(), b.fit_counts())

    for name, n, level in (("racks32", 1025, 0), ("four", 257, 1)):
        sc = SU.tree_scale_case(name, n, level)
        c, bt = sc.case, sc.case.batch
        for e in (a, b):
            SU.load_engine(e, sc)
            e.jobs_upload(fit_req, fit_need)               # staged before all of it
        scale_call(sc)
        J0 = len(c.job_domain)                              # the mix's own jobs, placed on both engines
        out = both(lambda e: e.place_greedy_domains(bt.job_group_off[:J0 + 1], bt.priority[:J0], bt.group_count, bt.group_req,
                                                    bt.group_need, c.job_domain, level, c.level_size, c.parent))
        assert np.array_equal(out[0][0], out[1][0]) and (out[0][1] == 0).any()
        scale_call(sc)
        donor = synth.make_inventory(2, 52, 0.5)
        free = [int(x) for x in np.setdiff1d(np.arange(n), np.concatenate([out[0][0], sc.gone]))[:2]]
        both(lambda e: e.update_nodes(free, [PE_NODE_SET, PE_NODE_SET], np.ascontiguousarray(donor.cap.T),
                                      np.ascontiguousarray(donor.used.T), donor.labels.copy(), c.island[free]))
        lab = np.array(c.labels, copy=True)
        lab[free] = synth.island_labels(donor.labels, c.island[free])
        moved = SU.ScaleCase(DP.Case(c.cap, c.used, lab, c.island, c.level_size, c.parent, level, bt, c.job_domain), sc.res,
                             sc.gone, *sc.call_args()[4:11])
        scale_call(moved)
        both(lambda e: e.reset_residuals())
        scale_call(moved)
    a.close()
    b.close()


def test_alternating_with_the_calls_that_share_its_buffers(eng):
    """pe_scale_up_domains, pe_gang_fit_domains and pe_drain_fit_domains in turn on one context, at sizes that grow
    and shrink the shared buffers."""
    for name, n, level in (("racks32", 1025, 1), ("four", 257, 0), ("fanin", 2500, 1)):
        sc = SU.tree_scale_case(name, n, level)
        SU.check_engine(eng, sc)
        c = sc.case
        island = np.where(sc.res[0] == SU.NEVER, -1, c.island)
        fits, fail, pods = GF.answers(sc.res, c.labels, island, c.batch, sc.pair_job, sc.pair_domain, level, c.level_size, c.parent)
        got = eng.gang_fit_domains(c.batch.job_group_off, c.batch.group_count, c.batch.group_req, c.batch.group_need,
                                   sc.pair_job, sc.pair_domain, level, c.level_size, c.parent)
        assert np.array_equal(got.fits, fits) and np.array_equal(got.fail_group, fail) and np.array_equal(got.pods, pods)
        SU.check_engine(eng, sc, load=False)
        DF.check_engine(eng, DF.tree_drain_case(name, n, level))
        SU.check_engine(eng, sc)


# ---------------------------------------------------------------- refusals

def test_refusals():
    n = 300
    island, sizes, parent = TC.tree("racks32", n)          # [10, 3, 1]
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    Q = [2000, 4 * GiB, 0, 0]
    jgo, cnt = [0, 1, 3], [2, 1, 3]
    req = np.array([Q, [8000, 32 * GiB, 1, 0], Q], dtype=np.int64)
    tres = np.array([[16000, 64 * GiB, 1, 0], [8000, 16 * GiB, 0, 0]], dtype=np.int64)
    good = dict(jgo=jgo, cnt=cnt, req=req, need=[0, 1, 0], tres=tres, tlab=[1, 3], slot=[7, 299, 100], pj=[0, 1, 1],
                pd=[1, 2, 9], pt=[0, 1, 1], pm=[3, 0, 2], level=0, sizes=sizes, parent=parent)
    outs = sentinels(3, 2)

    def refused(code, text, **change):
        rc, msg = raw(e, outs=outs, **dict(good, **change))
        assert rc == code and text in msg, (rc, msg, change)
        assert all((o == SENTINEL).all() for o in outs)

    refused(_abi.PE_ESTATE, "no inventory")                # before a load
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    e.update_nodes([7, 100, 299, 150], [PE_NODE_REMOVE] * 4)
    before, stats = e.read_residuals(), e.stats()
    E = _abi.PE_EINVAL
    bad_req = req.copy()
    bad_req[1, 2] = -1
    # what pe_gang_fit_domains refuses
    refused(E, "n_jobs < 0", n_jobs=-1)
    refused(E, "group_req", req=bad_req)
    refused(E, "group_count: negative value at index 1", cnt=[2, -1, 3])
    refused(E, "job_group_off", jgo=[0, 2, 1])
    refused(E, "pair_job or pair_domain is NULL", pj=None)
    refused(E, "pair_job or pair_domain is NULL", pd=None)
    refused(E, "n_pairs outside", n_pairs=-1)
    refused(E, "pair_job: value outside [0, n_jobs) at index 1", pj=[0, 2, 1])
    refused(E, "pair_domain: value outside [0, level_size[level]) at index 2", pd=[1, 2, 10])
    refused(E, "level outside", level=3)
    refused(E, "n_levels outside", n_levels=0)
    refused(E, "level_size is NULL", sizes=None, n_levels=3)
    refused(E, "level_size: value outside [1, PE_MAX_DOMAINS] at index 1", sizes=[10, 0, 1])
    refused(E, "parent is NULL", parent=None)
    # the templates
    refused(E, "n_templates < 0", n_templates=-1)
    refused(E, "n_templates < 0, or < 1 with pairs", n_templates=0)
    refused(E, "tmpl_res is NULL", tres=None, n_templates=2)
    bad_t = tres.copy()
    bad_t[1, 3] = -1
    refused(E, "tmpl_res: negative value in template at index 1", tres=bad_t)
    # the new slots
    refused(E, "n_new outside [0, PE_MAX_SCALE_NODES]", n_new=-1)
    refused(E, "n_new outside [0, PE_MAX_SCALE_NODES]", n_new=65)
    refused(E, "new_slot is NULL", slot=None, n_new=3)
    refused(E, "new_slot: value outside [0, n_total) at index 1", slot=[7, 300, 100])
    refused(E, "new_slot: value outside [0, n_total) at index 0", slot=[-1, 300, 100])
    refused(E, "new_slot: not a removed slot at index 2", slot=[7, 299, 101])
    refused(E, "new_slot: a slot named twice at index 2", slot=[7, 299, 7])
    # the pairs' templates and maxima
    refused(E, "pair_template is NULL", pt=None)
    refused(E, "pair_template: value outside [0, n_templates) at index 2", pt=[0, 1, 2])
    refused(E, "pair_template: value outside [0, n_templates) at index 0", pt=[-1, 1, 2])
    refused(E, "pair_max: value outside [0, n_new] at index 0", pm=[4, 0, 2])
    refused(E, "pair_max: value outside [0, n_new] at index 1", pm=[3, -1, 2])
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    # the same arguments unchanged are accepted, and the sentinels go
    rc, msg = raw(e, outs=outs, **good)
    assert rc == _abi.PE_OK, msg
    assert all((o != SENTINEL).all() for o in outs)
    batch = synth.JobBatch(np.array(jgo, dtype=np.int32), np.zeros(2, dtype=np.int32), np.array(cnt, dtype=np.int32), req,
                           np.array(good["need"], dtype=np.uint32), np.zeros(2, dtype=np.int8))
    case = DP.Case(inv.cap, inv.used, synth.island_labels(inv.labels, island), island, list(sizes), parent, 0, batch, None)
    col = lambda k: np.array(good[k], dtype=np.int32)   # noqa: E731
    sc = SU.ScaleCase(case, before, [7, 100, 299, 150], tres, np.array(good["tlab"], dtype=np.uint32), col("slot"), col("pj"),
                      col("pd"), col("pt"), col("pm"))
    assert all(np.array_equal(x, y) for x, y in zip(outs, SU.scale_oracle(sc)))
    with pytest.raises(PlacementError) as ei:              # the Python handle raises what the engine returns
        e.scale_up_domains(*sc.call_args()[:11], 7, sizes, parent)
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
        rc, msg = raw(s, [0, 1], [2], np.array([[2000, GiB, 0, 0]], dtype=np.int64), [0], np.array([[8000, GiB, 0, 0]]),
                      [1], [], [0], [0], [0], [0], 0, sizes, parent, outs)
        assert rc == _abi.PE_EINVAL and "shard" in msg
        assert all((o == SENTINEL).all() for o in outs) and np.array_equal(s.read_residuals(), before)
        s.close()
