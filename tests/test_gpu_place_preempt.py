"""pe_place_preempt_domains on the device against the rule stated sequentially in Python integers: gang_preempt.py's
two-phase procedure over the LIVE positions of a job's list, every judgement domain_placement.py's pod-by-pod
statement of the single job against the evolving residuals.  Every pod slot, status, prefix, mask, out_vic_job and
residual cell, exact."""
from types import SimpleNamespace

import numpy as np
import pytest

import domain_placement as DP
import gang_fit as GF
import gang_preempt as GP
from placement import PE_JOB_UNSCHEDULABLE, Engine, _abi, synth

pytestmark = pytest.mark.gpu

GiB, ISLAND, LDS = DP.GiB, DP.ISLAND, 1016          # pe_kernels.h PL_LDS_NODES
gpus, NEVER = GP.gpus, np.iinfo(np.int64).min


def rule(res, labels, island, batch, job_domain, level, level_size, parent, vic, jvo, jv):
    """(pods, status, prefix, mask, vic_job, residual [4][N]) by the header's rule, job by job."""
    R, dom = np.array(res, dtype=np.int64, copy=True), DP.dom_level(island, level, level_size, parent)
    pods_of, poff, J = [vic.pods(v) for v in range(len(vic))], DP.pod_offsets(batch.group_count), len(job_domain)
    pods, status = np.full(poff[-1], -1, dtype=np.int32), np.zeros(J, dtype=np.int32)
    prefix, mask, vic_job = np.full(J, -1, dtype=np.int32), np.zeros(J, dtype=np.uint64), np.full(len(vic), -1, dtype=np.int32)
    for j in sorted(range(J), key=lambda j: (-int(batch.priority[j]), j)):
        d, lst = int(job_domain[j]), [int(v) for v in jv[int(jvo[j]):int(jvo[j + 1])]]
        live = [i for i, v in enumerate(lst) if vic_job[v] < 0]         # a dead position releases nothing
        one, one_dom = DP.make_batch([(d, 0, GF.job_groups(batch, j))])
        seen = {}

        def judge(E):
            p, st, after, _ = DP.place_python(GP.released(R, dom, d, pods_of, [lst[live[i]] for i in E]), labels, island,
                                              one, one_dom, level, level_size, parent)
            seen[E] = (p, after)
            return st[0] == 0
        k, m, _ = GP.two_phase(judge, len(live))
        if k < 0:
            status[j] = PE_JOB_UNSCHEDULABLE
            continue
        E = tuple(i for i in range(len(live)) if m >> i & 1)
        a, b = poff[int(batch.job_group_off[j])], poff[int(batch.job_group_off[j + 1])]
        pods[a:b], R = seen[E][0], np.array(seen[E][1], dtype=np.int64)
        prefix[j], mask[j] = (live[k - 1] + 1 if k else 0), sum(1 << live[i] for i in E)
        vic_job[[lst[live[i]] for i in E]] = j
    for v in np.nonzero(vic_job >= 0)[0]:                                # the evicted gangs leave whole, afterwards
        for n, q in pods_of[v]:
            if dom[n] != job_domain[vic_job[v]] and R[0][n] != NEVER:
                R[:, n] += np.array(q, dtype=np.int64)
    return pods, status, prefix, mask, vic_job, R


def load(eng, c, vic):
    """The inventory with the victims assumed onto it: the reset snapshot is the one they can be released against."""
    own = np.zeros_like(c.used)
    for v in range(len(vic)):
        for n, q in vic.pods(v):
            own[:, n] += np.array(q, dtype=np.int64)
    eng.load_nodes(c.cap, c.used - own, c.labels, c.island)
    eng.assume_gangs(*vic.arrays())


def call(eng, c, vic, jvo, jv, dry_run=False):
    b = c.batch
    return eng.place_preempt_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, c.job_domain,
                                     c.level, c.level_size, c.parent, *vic.arrays(), jvo, jv, dry_run)


def check(eng, c, vic, jvo, jv, dry_run=False):
    before = eng.read_residuals()
    want = rule(before, c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent, vic, jvo, jv)
    got = call(eng, c, vic, jvo, jv, dry_run)
    for name, g, w in zip(("pods", "status", "prefix", "mask", "vic_job"), got, want):
        assert np.array_equal(g, w), (name, np.asarray(g).tolist()[:80], np.asarray(w).tolist()[:80])
    assert np.array_equal(eng.read_residuals(), before if dry_run else want[5])
    return SimpleNamespace(pods=want[0], status=want[1], prefix=want[2], mask=want[3], vic_job=want[4], res=want[5], before=before)


def lists(ls):
    return np.cumsum([0] + [len(x) for x in ls]).astype(np.int32), np.array([v for x in ls for v in x], dtype=np.int32)


def batch_case(size, seed=5):
    """Rack 0 of `size` nodes, rack 1 of two (gang_preempt.py's non-monotone trap), rack 2 of one, two nodes in no
    rack, ids shuffled.  In rack 0 only node t has GPUs (8: X 3, Y 1, Z 2, W 1 + 1 in two groups) and ephemeral storage
    (64: F0 .. F63 one each); the others have cpu alone.  W also holds 4 of the 8 GPUs of rack 2's node o."""
    ids = np.random.default_rng(seed).permutation(size + 5)
    r0, (a0, a1, o) = ids[:size], ids[size:size + 3]
    t, N = int(r0[0]), size + 5
    island = np.full(N, -1, dtype=np.int32)
    island[r0], island[[a0, a1]], island[o] = 0, 1, 2
    cap = np.array([[1000 + 7 * (i % 50) for i in range(N)], [64 * GiB] * N, [0] * N, [0] * N], dtype=np.int64)
    cap[:, t], cap[:, a0], cap[:, a1], cap[:, o] = [64000, 64 * GiB, 8, 64], [2000, 64 * GiB, 10, 0], [64000, 64 * GiB, 9, 0], [64000, 64 * GiB, 8, 0]
    vics = [(0, [(gpus(3), [t])]), (0, [(gpus(1), [t])]), (0, [(gpus(2), [t])]),                  # X Y Z
            (0, [(gpus(1), [t]), (gpus(4), [o, -1]), (gpus(1), [t])]),                            # W: t twice, o outside
            (0, [(gpus(5), [a1])]), (0, [(gpus(4), [a0])])] + [(0, [([0, 0, 0, 1], [t])]) for _ in range(64)]
    X, Y, Z, W, TX, TY, F = 0, 1, 2, 3, 4, 5, list(range(6, 70))
    vic = GP.make_victims(vics)
    used = np.zeros_like(cap)
    for v in range(len(vic)):
        for n, q in vic.pods(v):
            used[:, n] += np.array(q, dtype=np.int64)
    used[2, o] += 4                                                      # the rest of o: nobody's to evict
    jobs = [(0, 90, [(1, [1000, GiB, 0, 0], 0)], []),                                  # 0 fits, nobody evicted
            (0, 80, [(1, gpus(1), 0), (1, gpus(1), DP.NO_LABEL)], [X, Y]),            # 1 fails every prefix
            (0, 70, [(1, gpus(5, 100), 0)], [X, Y, Z]),                                # 2 reuses X: 0b101, Y comes back
            (0, 65, [(1, [0, 0, 0, 64], 0)], F),                                       # 3 the full mask of 64
            (0, 60, [(1, gpus(1), 0)], [X] + F[:60] + [Z, Y]),                         # 4 62 dead positions, then Y
            (0, 50, [(2, gpus(1), ISLAND)], [Z, W]),                                   # 5 an island; a dead position k - 1
            (0, 20, [(1, gpus(1), 0)], [Y]),                                           # 6 its only candidate is dead
            (1, 9, [(1, gpus(5, 1000, GiB), 0), (1, gpus(5, 32000, GiB), 0)], [TX, TY]),   # 7 the trap: no, yes, no
            (2, 1, [(1, gpus(4), 0)], [])]                                             # 8 must not see W's 4 GPUs on o
    batch, job_domain = DP.make_batch([j[:3] for j in jobs])
    case = DP.Case(cap, used, synth.island_labels(np.ones(N, dtype=np.uint32), island), island, [3], None, 0, batch, job_domain)
    return case, vic, lists([j[3] for j in jobs]), o


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("size", [1, 255, 257, LDS - 1, LDS, LDS + 1])
def test_against_the_rule(eng, size):
    c, vic, (jvo, jv), o = batch_case(size)
    load(eng, c, vic)
    w = check(eng, c, vic, jvo, jv, dry_run=True)                        # the dry run, then the committed call
    assert np.array_equal(check(eng, c, vic, jvo, jv).pods, w.pods)
    # the batch shows what it was made for, by the reference alone
    assert w.status.tolist() == [0, 1, 0, 0, 0, 0, 1, 0, 1] and w.prefix.tolist() == [0, -1, 3, 64, 63, 2, -1, 1, -1]
    assert [int(m) for m in w.mask] == [0, 0, 0b101, 2**64 - 1, 1 << 62, 0b10, 0, 0b01, 0]
    assert w.vic_job[:6].tolist() == [2, 4, 2, 5, 7, -1] and (w.vic_job[6:] == 3).all()
    assert w.before[2][o] == 0 and w.res[2][o] == 4                      # W's pod outside rack 0: after the call only
    # ledger closure: the placed jobs released, the evicted victims assumed, and the residuals are back
    b = c.batch
    eng.release_gangs(b.job_group_off, b.group_count, b.group_req, w.pods)
    evicted = np.repeat(np.repeat(w.vic_job >= 0, np.diff(vic.group_off)), vic.group_count)
    eng.assume_gangs(vic.group_off, vic.group_count, vic.group_req, np.where(evicted, vic.pod_node, -1))
    assert np.array_equal(eng.read_residuals(), w.before)


def test_worked_example(eng):
    cap = np.array([[64000] * 2, [256 << 30] * 2, [8] * 2, [0] * 2], dtype=np.int64)
    vic = GP.make_victims([(0, [(gpus(4), [0])]), (0, [(gpus(4), [0])]), (0, [(gpus(8), [1])])])   # A B C
    batch, dom = DP.make_batch([(0, 10, [(1, gpus(8), 0)]), (0, 5, [(1, gpus(4), 0)])])
    c = DP.Case(cap, np.array([[0] * 2, [0] * 2, [8] * 2, [0] * 2], dtype=np.int64), np.ones(2, dtype=np.uint32),
                np.zeros(2, dtype=np.int32), [1], None, 0, batch, dom)
    load(eng, c, vic)
    w = check(eng, c, vic, *lists([[0, 2, 1], [2, 0]]))
    assert (w.pods.tolist(), w.prefix.tolist(), [int(m) for m in w.mask], w.vic_job.tolist()) == ([1, 0], [2, 2], [0b010, 0b10], [1, -1, 0])
    assert w.res[2].tolist() == [0, 0]


def test_identity_empty_lists_is_place_greedy_domains(eng):
    other = Engine(0)
    for level in (0, 2):
        c = DP.tree_case("racks32", 1025, level)
        for e in (eng, other):
            e.load_nodes(c.cap, c.used, c.labels, c.island)
        b = c.batch
        want = other.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                          c.job_domain, level, c.level_size, c.parent)
        got = call(eng, c, GP.make_victims([]), np.zeros(len(c.job_domain) + 1, dtype=np.int32), [])
        assert np.array_equal(got.pod_node, want[0]) and np.array_equal(got.status, want[1]) and (want[1] == 0).any()
        assert np.array_equal(got.prefix, -want[1]) and not got.victims.any()
        assert np.array_equal(eng.read_residuals(), other.read_residuals())
    other.close()


@pytest.mark.parametrize("trap", list(GP.TRAPS))
def test_identity_one_job_is_gang_preempt_domains(eng, trap):
    pc, _ = GP.TRAPS[trap]()
    c, b = pc.case, pc.case.batch
    for p in range(len(pc.pair_job)):
        j, lst = int(pc.pair_job[p]), pc.pair_vic[int(pc.pair_vic_off[p]):int(pc.pair_vic_off[p + 1])]
        load(eng, c, pc.vic)
        pre = eng.gang_preempt_domains(*pc.call_args())
        one, _ = DP.make_batch([(0, 0, GF.job_groups(b, j))])
        got = eng.place_preempt_domains(one.job_group_off, one.priority, one.group_count, one.group_req, one.group_need,
                                        [int(pc.pair_domain[p])], c.level, c.level_size, c.parent, *pc.vic.arrays(),
                                        [0, len(lst)], lst, dry_run=bool(p & 1))
        assert (got.prefix[0], got.victims[0]) == (pre.prefix[p], pre.victims[p])


def test_refusals():
    c, vic, (jvo, jv), _ = batch_case(3)
    b, J, V = c.batch, len(c.job_domain), len(vic)
    long_jvo, two, dup, big = jvo.copy(), jv.copy(), jv.copy(), vic.group_req.copy()
    long_jvo[1:] += 65                                                   # job 0's list: victims 0 .. 64
    two[int(jvo[8]) - 1] = 0                                             # X in the trap's list too: racks 0 and 1
    dup[1], big[0] = dup[0], gpus(4)                                     # X gives back 4 of the 3 GPUs it took
    outs = [np.full(n, 77, dtype=t) for n, t in ((16, np.int32), (J, np.int32), (J, np.int32), (J, np.uint64), (V, np.int32))]

    def answers(e, code, text, n_jobs=J, jvo=jvo, jv=jv, req=vic.group_req, flags=0):
        arrs = [b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, c.job_domain,
                np.array(c.level_size, dtype=np.int32), vic.group_off, vic.group_count, req, vic.pod_node, jvo, jv]
        k = [np.ascontiguousarray(a).ctypes.data for a in arrs]
        rc = e.lib.pe_place_preempt_domains(e.h, n_jobs, *k[:6], 0, 1, k[6], None, V, *k[7:13], flags, *[x.ctypes.data for x in outs])
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert all((x == 77).all() for x in outs) == (code != _abi.PE_OK)   # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    load(e, c, vic)
    before, E = e.read_residuals(), _abi.PE_EINVAL
    answers(e, E, "n_jobs < 0", n_jobs=-1)
    answers(e, E, "two domains at index %d" % (int(jvo[8]) - 1), jv=two)
    answers(e, E, "the same victim twice in one list at index 1", jv=dup)
    answers(e, E, "PE_MAX_PAIR_VICTIMS candidate victims for the job at index 0", jvo=long_jvo,
            jv=np.concatenate([np.arange(65, dtype=np.int32), jv]))
    answers(e, E, "more than was taken", req=big)
    answers(e, E, "flags: unknown bits", flags=2)
    assert np.array_equal(e.read_residuals(), before)
    for r in range(2):                                                   # a 2-shard context
        s = Engine(0, rank=r, world_size=2, exchange=lambda x: x * 2)
        s.load_nodes(c.cap, c.used, c.labels, c.island)
        answers(s, E, "shard")
        s.close()
    answers(e, _abi.PE_OK, "", flags=1)                                  # the same arguments are accepted
    e.close()

