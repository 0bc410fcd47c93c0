"""Checker for pe_place_first_fit_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): jobs in (priority desc, index asc) order; job j tries its candidates -- its pairs
in ascending p -- in order; an attempt at pair p is pe_place_greedy_domains on the single job j with job_domain =
pair_domain[p] against the residuals as every earlier job left them; the first attempt that is placed stands, a
failed one is rolled back in full; a job whose candidates all fail, or that is in no pair, is unschedulable with -1
in all its pod slots.  Three statements of it:

    place_first_fit(...)         the sequential rule, every attempt one domain_placement.place (the C oracle) on
                                 the single job
    place_first_fit_python(...)  the same loop through domain_placement.place_python (small inputs)
    rounds_model(...)            the device's round scheme restated in Python: per active
                                 domain a queue of (job, k) entries sorted by (rank, k), per job the position of the
                                 candidate it tries next, rounds in which every domain works off the head of its
                                 queue against the jobs' state AS THE ROUND BEGAN; returns the rounds it took as well

An attempt touches the nodes of its candidate domain only, so each statement hands domain_placement the
sub-inventory of that domain (ascending global ids -> ascending local ids, which preserves the key order) and
maps the local ids back.

`labels` are the engine's labels: synth.island_labels applied.
"""
import numpy as np

import domain_placement as DP
import gang_fit as GF
from placement import synth

GiB = 1 << 30


def job_order(priority):
    return sorted(range(len(priority)), key=lambda j: (-int(priority[j]), j))


def candidates(pair_job, J):
    """[[p, ...] ascending] per job."""
    out = [[] for _ in range(J)]
    for p, j in enumerate(pair_job):
        out[int(j)].append(p)
    return out


def single_job(batch, j):
    """The batch of job j alone."""
    g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
    return synth.JobBatch(np.array([0, g1 - g0], dtype=np.int32), np.asarray(batch.priority)[j:j + 1],
                          np.asarray(batch.group_count)[g0:g1], np.asarray(batch.group_req).reshape(-1, 4)[g0:g1],
                          np.asarray(batch.group_need)[g0:g1], np.zeros(1, dtype=np.int8))


class _Attempts:
    """One attempt = domain_placement's placement of a single job in one domain, on the evolving residuals."""

    def __init__(self, res, labels, island, batch, level, level_size, parent, python):
        self.res = np.array(res, dtype=np.int64, copy=True)
        self.labels = np.asarray(labels, dtype=np.uint32)
        self.island = np.asarray(island)
        self.batch = batch
        self.level, self.level_size, self.parent = level, level_size, parent
        self.members = GF.members_of(island, level, level_size, parent)
        self.python = python
        self.poff = DP.pod_offsets(batch.group_count)
        self.pods = np.full(self.poff[-1], -1, dtype=np.int32)

    def attempt(self, j, d):
        """Tries job j in domain d; on success its pods and the residuals are kept.  Returns whether it was placed."""
        nodes = self.members.get(int(d), np.zeros(0, dtype=np.int64))
        one = single_job(self.batch, j)
        place = DP.place_python if self.python else DP.place
        out = place(self.res[:, nodes], self.labels[nodes], self.island[nodes], one, np.array([d], dtype=np.int32),
                    self.level, self.level_size, self.parent)
        pods, status, after = np.asarray(out[0], dtype=np.int64), out[1], np.array(out[2], dtype=np.int64).reshape(4, -1)
        if int(status[0]) != 0:
            assert (pods == -1).all() and np.array_equal(after, self.res[:, nodes])     # rolled back in full
            return False
        self.res[:, nodes] = after
        p0 = self.poff[int(self.batch.job_group_off[j])]
        self.pods[p0:p0 + len(pods)] = nodes[pods] if len(pods) else pods
        return True


def _first_fit(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent, python):
    J = len(batch.job_group_off) - 1
    at = _Attempts(res, labels, island, batch, level, level_size, parent, python)
    cand = candidates(pair_job, J)
    status = np.ones(J, dtype=np.int32)
    pair = np.full(J, -1, dtype=np.int32)
    for j in job_order(batch.priority):
        for p in cand[j]:
            if at.attempt(j, int(pair_domain[p])):
                status[j], pair[j] = 0, p
                break
    return at.pods, status, pair, at.res


def place_first_fit(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent):
    """(pod_node int32[P], job_status int32[J], job_pair int32[J], residual_after int64[4][N]): the sequential rule."""
    return _first_fit(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent, False)


def place_first_fit_python(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent):
    return _first_fit(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent, True)


def rounds_model(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent, reverse=False):
    """place_first_fit's outputs by the round scheme, plus the number of rounds.  reverse: the domains take their
    turn within a round in descending order -- the answer and the rounds must not depend on it."""
    J = len(batch.job_group_off) - 1
    at = _Attempts(res, labels, island, batch, level, level_size, parent, False)
    cand = candidates(pair_job, J)
    rank = {j: i for i, j in enumerate(job_order(batch.priority))}
    queue = {}
    for j in range(J):
        for k, p in enumerate(cand[j]):
            queue.setdefault(int(pair_domain[p]), []).append((rank[j], k, j, p))
    for q in queue.values():
        q.sort()
    cursor = {d: 0 for d in queue}
    ptr, settled = [0] * J, [not cand[j] for j in range(J)]
    status = np.ones(J, dtype=np.int32)
    pair = np.full(J, -1, dtype=np.int32)
    rounds = 0
    while not all(settled):
        rounds += 1
        assert rounds <= len(pair_job) + 1, "the round scheme did not terminate within n_pairs + 1 rounds"
        ptr0, settled0 = list(ptr), list(settled)        # the jobs' state as the round began
        touched = set()                                  # the jobs attempted in this round (their stamp is this round's)
        for d in sorted(queue, reverse=reverse):
            q = queue[d]
            while cursor[d] < len(q):
                _, k, j, p = q[cursor[d]]
                if settled0[j] or ptr0[j] > k:
                    cursor[d] += 1
                    continue
                if ptr0[j] < k or j in touched:
                    break
                touched.add(j)
                cursor[d] += 1
                if at.attempt(j, d):
                    status[j], pair[j], settled[j] = 0, p, True
                elif k + 1 == len(cand[j]):
                    settled[j] = True
                else:
                    ptr[j] = k + 1
    return at.pods, status, pair, at.res, rounds


# ---------------------------------------------------------------- shared inputs

def add_jobs(case, jobs):
    """The case with jobs (domain_placement.make_batch's triples) appended to its batch."""
    b, (more, dom) = case.batch, DP.make_batch(jobs)
    batch = synth.JobBatch(np.concatenate([b.job_group_off, more.job_group_off[1:] + b.job_group_off[-1]]).astype(np.int32),
                           np.concatenate([b.priority, more.priority]), np.concatenate([b.group_count, more.group_count]),
                           np.concatenate([np.asarray(b.group_req).reshape(-1, 4), more.group_req]),
                           np.concatenate([b.group_need, more.group_need]), np.concatenate([b.kind, more.kind]))
    return DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, case.parent, case.level, batch,
                   np.concatenate([case.job_domain, dom]).astype(np.int32))


def pair_lists(case, seed, res=None):
    """(case with four more jobs, pair_job, pair_domain) for a domain_placement.Case.  gang_fit.pair_mix's lists
    for the job mix (an empty domain, two other domains, the job's own domain twice; dealt over shuffled positions),
    with every pair of the mix's last job taken out -- a job in no pair -- and, appended, the traps every case must
    show whatever its level: in the domain d with the most nodes, H (the highest priority) takes every node that
    holds a pod of the largest cpu residual, L (next priority, one such pod, candidates [d]) would fit alone and
    finds nothing, N needs a label no node has and fails every one of its candidates, and M (one such pod again) is
    placed by its second pair where the level has a second domain.  res: the residuals to size the traps against
    (default: the case's own)."""
    pj, pd = GF.pair_mix(case, seed)
    J = len(case.batch.job_group_off) - 1
    keep = pj != J - 1
    pj, pd = pj[keep], pd[keep]
    res = case.residual() if res is None else np.asarray(res)
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    d = int(np.bincount(dom[dom >= 0]).argmax())
    mine = (dom == d) & (res >= 0).all(axis=0)
    top = int(res[0][mine].max())
    assert top > 0
    q = [top, 0, 0, 0]
    n_top = int((res[0][mine] >= top).sum())
    others = [int(x) for x in np.unique(dom[dom >= 0]) if x != d]
    usable = (res >= 0).all(axis=0)
    roomy = [o for o in others if (res[0][(dom == o) & usable] >= top).any()]
    if roomy:       # M comes after H, finds d full and goes on to a domain that holds its pod
        m_pri, m_list = 997, [d, roomy[0]]
    elif others:    # M comes first, finds no such node elsewhere and takes one of d's: one fewer for H
        m_pri, m_list, n_top = 1001, [others[0], d], n_top - 1
    else:           # a level of one domain: every pair names it, and no later pair can do what the first could not
        m_pri, m_list = 997, [d]
    case = add_jobs(case, [(d, 1000, [(n_top, q, 0)]), (d, 999, [(1, q, 0)]), (d, 998, [(1, [1, 0, 0, 0], DP.NO_LABEL)]),
                           (d, m_pri, [(1, q, 0)])])
    n_list = others[:2] + [d]
    pj = np.concatenate([pj, [J, J + 1] + [J + 2] * len(n_list) + [J + 3] * len(m_list)]).astype(np.int32)
    pd = np.concatenate([pd, [d, d] + n_list + m_list]).astype(np.int32)
    return case, pj, pd


def pairs_case(name, n, level, seed=67):
    return pair_lists(DP.tree_case(name, n, level), seed + 13 * level + n)


def gpu_case(domains, jobs):
    """A hand-made one-level case: domains = [[free GPUs of each node], ...] (every node with 64 cores and 256 GiB
    free), jobs = [(priority, [(count, gpus per pod), ...], [candidate domain, ...]), ...].  A job's pairs are
    contiguous, the jobs' lists in job order.  Returns (Case, pair_job, pair_domain); job_domain is unused."""
    island = np.array([d for d, nodes in enumerate(domains) for _ in nodes], dtype=np.int32)
    gpus = [g for nodes in domains for g in nodes]
    n = len(gpus)
    cap = np.array([[64000] * n, [256 * GiB] * n, gpus, [0] * n], dtype=np.int64)
    labels = synth.island_labels(np.ones(n, dtype=np.uint32), island)
    batch, _ = DP.make_batch([(0, pri, [(c, [1000, GiB, g, 0], 0) for c, g in groups]) for pri, groups, _ in jobs])
    pj = [j for j, (_, _, cands) in enumerate(jobs) for _ in cands]
    pd = [d for _, _, cands in jobs for d in cands]
    case = DP.Case(cap, np.zeros_like(cap), labels, island, [len(domains)], None, 0, batch, np.zeros(len(jobs), dtype=np.int32))
    return case, np.array(pj, dtype=np.int32), np.array(pd, dtype=np.int32)


def trap_priority():
    """Domain 1 has one GPU, domain 2 four.  B (job 0, low priority) wants 4 GPUs in [2]; A (job 1, high priority)
    wants 4 GPUs in [1, 2] and fails in 1.  A is placed in 2 by its second pair (pair 2) and B is unschedulable; a
    scheme that lets every job propose at once places B."""
    return gpu_case([[0], [1], [4]], [(0, [(1, 4)], [2]), (9, [(1, 4)], [1, 2])])


TRAP_PRIORITY_WANT = dict(pods=[-1, 2], status=[1, 0], pair=[-1, 2])


def trap_chain():
    """Domains 0 .. 4 have one GPU each, domain 5 eight.  X (job 0, high priority, 2 GPUs) fails five candidates and
    fits the sixth; behind it queue L0 .. L4 (1 GPU, [i]), which are placed once X has moved on, and L5 (8 GPUs,
    [5]), which finds 6 GPUs left."""
    jobs = [(9, [(1, 2)], [0, 1, 2, 3, 4, 5])] + [(0, [(1, 1)], [i]) for i in range(5)] + [(0, [(1, 8)], [5])]
    return gpu_case([[1]] * 5 + [[8]], jobs)


TRAP_CHAIN_WANT = dict(pods=[5, 0, 1, 2, 3, 4, -1], status=[0] * 6 + [1], pair=[5, 6, 7, 8, 9, 10, -1], rounds=6)


def trap_repeat():
    """include/placement.h's two-node rack (domain 0: 8 + 8 GPUs) and a rack of three such nodes (domain 1).  A
    (2 x 5 GPUs, then 3 x 2) lists [0, 0, 1]: it takes four pods in domain 0 and fails, twice, then fits domain 1.
    B (low priority, 2 x 8 GPUs, [0]) fits only if both rollbacks gave everything back."""
    return gpu_case([[8, 8], [8, 8, 8]], [(9, [(2, 5), (3, 2)], [0, 0, 1]), (0, [(2, 8)], [0])])


TRAP_REPEAT_WANT = dict(status=[0, 0], pair=[2, 3])


def trap_all_one_domain(n_jobs=200):
    """n_jobs jobs that all name domain 0 only (40 synth nodes; domain 1 is never named): one queue, one round."""
    rng = np.random.default_rng(5)
    jobs = [(0, int(rng.integers(0, 3)), [(int(rng.integers(1, 9)), [int(rng.choice(DP._CPU)), int(rng.choice(DP._MEM)), 0, 0], 0)])
            for _ in range(n_jobs)]
    case = DP.one_level_case([40, 9], jobs, seed=43)
    return case, np.arange(n_jobs, dtype=np.int32), np.zeros(n_jobs, dtype=np.int32)


def overflow_case(big, seed=71, n_jobs=28):
    """One level: domain 0 with `big` nodes beside domains 1 and 2 with 6 and 9.  Every fourth job is a GPU job of
    one to three pods whose list starts in the large domain, where the highest-priority job G has taken every free
    GPU: it overflows into the small domains.  The others are sized against what the first domain of their list
    holds, with lists that start in the large domain and go on to the small ones or the other way round, some
    with repeats: the ones that the small domains refuse come back to the large one."""
    sizes = [big, 6, 9]
    case = DP.one_level_case(sizes, [], seed=seed)
    res = case.residual()
    dom = DP.dom_level(case.island, 0, case.level_size, None)
    q = [2000, 4 * GiB, 0, 0]
    ok = (res >= 0).all(axis=0)
    per = np.where(ok, np.minimum(res[0] // q[0], res[1] // q[1]), 0)
    slots = [int(per[dom == d].sum()) for d in range(3)]
    rng = np.random.default_rng(seed + big)
    lists = [[1, 0], [2, 1, 0], [0, 1, 2], [1, 2, 0], [2, 0], [0, 1], [1], [0]]
    gpu_lists = [[0, 1, 2], [0, 0, 2], [0, 2, 1]]
    jobs = [(0, 100, [(int(res[2][ok & (dom == 0)].sum()), [0, 0, 1, 0], 0)])]
    cands = [[0]]
    for i in range(1, n_jobs):
        if i % 4 == 0:
            c = gpu_lists[(i // 4) % len(gpu_lists)]
            groups = [(int(rng.integers(1, 4)), [500, GiB, 1, 0], 0)]
        else:
            c = lists[i % len(lists)]
            groups = [(max(1, int(slots[0] * rng.choice([0.15, 0.3, 0.45]))), q, 0)]
        if i % 5 == 0:
            groups.append((2, [500, GiB, 0, 0], DP.ISLAND))
        jobs.append((0, int(rng.integers(0, 4)) + (4 if c[0] else 0), groups))    # the small domains' jobs first
        cands.append(c)
    batch, _ = DP.make_batch(jobs)
    case = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, None, 0, batch,
                   np.zeros(n_jobs, dtype=np.int32))
    owner = rng.permutation(np.repeat(np.arange(n_jobs), [len(c) for c in cands]))
    at = [0] * n_jobs
    pd = []
    for j in owner:
        pd.append(cands[j][at[j]])
        at[j] += 1
    return case, owner.astype(np.int32), np.array(pd, dtype=np.int32)


def overflow_conditions(pair_job, pair_domain, pair):
    """(some job was placed in a small domain after the large one refused it, some job was placed in the large
    domain after a small one refused it) on an answer's job_pair."""
    cand = candidates(pair_job, len(pair))
    out, back = False, False
    for j, p in enumerate(pair):
        if p < 0:
            continue
        before = [int(pair_domain[x]) for x in cand[j] if x < p]
        out |= int(pair_domain[p]) != 0 and 0 in before
        back |= int(pair_domain[p]) == 0 and any(d != 0 for d in before)
    return out, back


def check_engine(eng, case, pair_job, pair_domain, load=True, python=False, want=None):
    """Load the case (unless the engine already holds it), run the call and compare every pod slot, status, job
    pair and residual cell with the checker -- and with the Python statement too where asked (small inputs).
    Returns the checker's (pods, status, pair, residual)."""
    if load:
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before = eng.read_residuals()
    b = case.batch
    args = (before, case.labels, case.island, b, pair_job, pair_domain, case.level, case.level_size, case.parent)
    if want is None:
        want = place_first_fit(*args)
    pods, st, pair = eng.place_first_fit_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                                 pair_job, pair_domain, case.level, case.level_size, case.parent)
    assert np.array_equal(st, want[1]), (st.tolist(), want[1].tolist())
    assert np.array_equal(pair, want[2]), (pair.tolist(), want[2].tolist())
    assert np.array_equal(pods, want[0])
    assert np.array_equal(eng.read_residuals(), want[3])
    if python:
        py = place_first_fit_python(*args)
        assert np.array_equal(pods, py[0]) and np.array_equal(st, py[1]) and np.array_equal(pair, py[2])
        assert np.array_equal(eng.read_residuals(), py[3])
    return want
