"""Checker for pe_gang_fit_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): pair p asks whether pe_place_greedy_domains, given the single job pair_job[p] with
job_domain = pair_domain[p] against the current residuals, would place it.  Two statements of it:

    fits_oracle(...)   per pair, domain_placement.place (the C oracle on the domain's sub-inventory) with the
                       single job on a copy of the residuals: fits = (status == 0)
    fit_python(...)    domain_placement.place_python's loop restated for one job, one pod at a time in Python
                       integers (small inputs); it stops at the first pod without a node and returns
                       (fits, fail_group, pods)

and, for inputs too large for the Python statement, answers(...): fail_group and pods from the oracle alone.  The
rule places pod after pod and never takes one back before the job fails, so a job fails at group g iff the job cut
after group g fails and the job cut after group g - 1 does not, and it had placed c pods of group g iff the job
cut to c pods of group g is placed and the one cut to c + 1 is not: a walk over the groups and a bisection over
the count, each step one oracle call.

`labels` are the engine's labels: synth.island_labels applied.
"""
import numpy as np

import domain_placement as DP
import oracle
from oracle import semantics as S

ISLAND = DP.ISLAND


def job_groups(batch, j):
    """[(count, request[4], need), ...] of job j."""
    g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
    return [(int(batch.group_count[g]), [int(x) for x in batch.group_req[g]], int(batch.group_need[g])) for g in range(g0, g1)]


def members_of(island, level, level_size, parent):
    """{domain: ascending node ids} of the hierarchy's `level`."""
    dom = DP.dom_level(island, level, level_size, parent)
    return {int(d): np.nonzero(dom == d)[0] for d in np.unique(dom) if d >= 0}


def placed_alone(res, labels, nodes, groups):
    """Whether the C oracle places the one job `groups` on the sub-inventory of `nodes` (ascending global ids ->
    ascending local ids, which preserves the key order): domain_placement.place's step for one domain and one job."""
    if not any(c > 0 for c, _, _ in groups):
        return True                                         # nothing to place: placed, nodes or not
    if len(nodes) == 0:
        return False
    cnt = np.array([c for c, _, _ in groups], dtype=np.int32)
    req = np.array([q for _, q, _ in groups], dtype=np.int64).reshape(-1, 4)
    need = np.array([nd for _, _, nd in groups], dtype=np.uint32)
    _, st, _ = oracle.place_greedy(np.asarray(res)[:, nodes], np.asarray(labels)[nodes], np.array([0, len(groups)], dtype=np.int32),
                                   np.zeros(1, dtype=np.int32), cnt, req, need)
    return int(st[0]) == 0


def fits_oracle(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent):
    """uint8[P]: per pair, the single job placed by the C oracle on its domain's sub-inventory."""
    members = members_of(island, level, level_size, parent)
    none = np.zeros(0, dtype=np.int64)
    memo = {}
    out = np.zeros(len(pair_job), dtype=np.uint8)
    for p, (j, d) in enumerate(zip(pair_job, pair_domain)):
        key = (int(j), int(d))
        if key not in memo:
            memo[key] = placed_alone(res, labels, members.get(int(d), none), job_groups(batch, int(j)))
        out[p] = memo[key]
    return out


def answer_oracle(res, labels, nodes, groups):
    """(fits, fail_group, pods) of one job on one domain's nodes, from the oracle alone (the module's docstring)."""
    if placed_alone(res, labels, nodes, groups):
        return 1, -1, sum(max(c, 0) for c, _, _ in groups)
    g = next(k for k in range(len(groups)) if not placed_alone(res, labels, nodes, groups[:k + 1]))
    c, q, nd = groups[g]
    before = sum(max(x, 0) for x, _, _ in groups[:g])
    if nd & ISLAND:
        return 0, g, before                                 # one unit: none of its pods
    lo, hi = 0, c                                           # lo pods of group g are placed, hi are not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if placed_alone(res, labels, nodes, groups[:g] + [(mid, q, nd)]):
            lo = mid
        else:
            hi = mid
    return 0, g, before + lo


def answers(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent):
    """(fits uint8[P], fail_group int32[P], pods int64[P]) of every pair, by answer_oracle."""
    members = members_of(island, level, level_size, parent)
    none = np.zeros(0, dtype=np.int64)
    memo = {}
    P = len(pair_job)
    fits, fail, pods = np.zeros(P, dtype=np.uint8), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int64)
    for p, (j, d) in enumerate(zip(pair_job, pair_domain)):
        key = (int(j), int(d))
        if key not in memo:
            memo[key] = answer_oracle(res, labels, members.get(int(d), none), job_groups(batch, int(j)))
        fits[p], fail[p], pods[p] = memo[key]
    return fits, fail, pods


def fit_python(res, labels, nodes, groups):
    """(fits, fail_group, pods): domain_placement.place_python's loop for one job confined to `nodes`, one pod at a
    time in Python integers, stopped at the first pod that finds no node."""
    R = {int(n): [int(res[d][n]) for d in range(4)] for n in nodes}
    lab = {int(n): int(labels[n]) for n in nodes}

    def argmin(q, need):
        best = None
        for n, r in R.items():
            k = S.appendix_b_key(r, lab[n], q, need, n)
            if k is not None and (best is None or k < best):
                best = k
        return best

    pods = 0
    for g, (c, q, need) in enumerate(groups):
        if need & ISLAND and c > 0:
            qe = [x * c for x in q]
            best = argmin(qe, need) if all(v <= S.INT64_MAX for v in qe) else None
            if best is None:
                return 0, g, pods
            n = best & 0xFFFFFF
            R[n] = [r - v for r, v in zip(R[n], qe)]
            pods += c
            continue
        for _ in range(c):
            best = argmin(q, need)
            if best is None:
                return 0, g, pods
            n = best & 0xFFFFFF
            R[n] = [r - v for r, v in zip(R[n], q)]
            pods += 1
    return 1, -1, pods


def answers_python(res, labels, island, batch, pair_job, pair_domain, level, level_size, parent):
    """answers(...) by fit_python."""
    members = members_of(island, level, level_size, parent)
    memo = {}
    P = len(pair_job)
    fits, fail, pods = np.zeros(P, dtype=np.uint8), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int64)
    for p, (j, d) in enumerate(zip(pair_job, pair_domain)):
        key = (int(j), int(d))
        if key not in memo:
            memo[key] = fit_python(res, labels, members.get(int(d), []), job_groups(batch, int(j)))
        fits[p], fail[p], pods[p] = memo[key]
    return fits, fail, pods


def first_of(pair_job, fits, J):
    """int32[J]: the smallest p with pair_job[p] == j and fits[p], -1 when there is none."""
    first = np.full(J, -1, dtype=np.int32)
    for p in range(len(pair_job) - 1, -1, -1):
        if fits[p]:
            first[int(pair_job[p])] = p
    return first


# ---------------------------------------------------------------- shared inputs

def pair_mix(case, seed):
    """(pair_job, pair_domain) int32[P] for a domain_placement.Case.  For every job of its job_mix, in this order:
    an empty domain (where the level has one), two other populated domains (where the level has them: the one with
    the fewest nodes, which holds few gangs, and a random one), then its own domain twice -- the likeliest fit
    last, so that first fit has something to skip.  The jobs' lists are dealt over shuffled positions: the pairs are
    not grouped by job, and a job's order among its own pairs is kept."""
    rng = np.random.default_rng(seed)
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    n_dom = int(case.level_size[case.level])
    size = np.bincount(dom[dom >= 0], minlength=n_dom)
    populated, empty = np.nonzero(size > 0)[0], np.nonzero(size == 0)[0]
    smallest = int(populated[size[populated].argmin()]) if len(populated) else -1
    lists = []
    for own in (int(d) for d in case.job_domain):
        others = [d for d in [smallest] + [int(d) for d in rng.permutation(populated)] if d not in (own, -1)]
        lists.append(([int(rng.choice(empty))] if len(empty) else []) + list(dict.fromkeys(others))[:2] + [own, own])
    owner = rng.permutation(np.repeat(np.arange(len(lists)), [len(x) for x in lists]))   # whose pair each position is
    at = [0] * len(lists)
    pair_domain = []
    for j in owner:
        pair_domain.append(lists[j][at[j]])
        at[j] += 1
    return owner.astype(np.int32), np.array(pair_domain, dtype=np.int32)


def pairs_case(name, n, level, seed=53):
    """(domain_placement.tree_case(name, n, level), pair_job, pair_domain)."""
    case = DP.tree_case(name, n, level)
    return (case,) + pair_mix(case, seed + 11 * level + n)


def check_engine(eng, case, pair_job, pair_domain, load=True, python=False):
    """Load the case (unless the engine already holds it), run the call and compare every fits, fail_group, pods
    and first cell with the checker (the oracle statement) -- and fits with the Python statement too where asked
    (small inputs).  The
    residuals must come out as they went in.  Returns the checker's (fits, fail_group, pods, first)."""
    if load:
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before = eng.read_residuals()
    b = case.batch
    args = (before, case.labels, case.island, b, pair_job, pair_domain, case.level, case.level_size, case.parent)
    fits, fail, pods = answers(*args)
    first = first_of(pair_job, fits, len(b.job_group_off) - 1)
    got = eng.gang_fit_domains(b.job_group_off, b.group_count, b.group_req, b.group_need, pair_job, pair_domain, case.level,
                               case.level_size, case.parent)
    assert np.array_equal(got.fits, fits), np.nonzero(got.fits != fits)[0][:10].tolist()
    assert np.array_equal(got.fail_group, fail), np.nonzero(got.fail_group != fail)[0][:10].tolist()
    assert np.array_equal(got.pods, pods), np.nonzero(got.pods != pods)[0][:10].tolist()
    assert np.array_equal(got.first, first)
    if python:
        assert np.array_equal(got.fits, answers_python(*args)[0])
    assert np.array_equal(eng.read_residuals(), before)
    return fits, fail, pods, first
