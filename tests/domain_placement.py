"""Checker for pe_place_greedy_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): pe_place_greedy's, with one more condition in fit -- job j's pods land only on
nodes whose level-`level` domain is job_domain[j].  Two statements of it:

    place(...)         per active domain, the C oracle (oracle.place_greedy) on the sub-inventory of the domain's
                       nodes (ascending global id -> ascending local id, which preserves the key order) with the
                       domain's jobs; local ids mapped back, pods, statuses and residuals stitched together
    place_python(...)  semantics.place_greedy_appendix_b's loop restated with the domain condition in the fit,
                       one pod at a time in Python integers (small inputs); it also reports every rollback

`labels` are the engine's labels: synth.island_labels applied.
"""
from dataclasses import dataclass

import numpy as np

import domain_capacity as DC
import tree_capacity as TC
import oracle
from oracle import semantics as S
from placement import synth

GiB = 1 << 30
ISLAND = 1 << 31
NO_LABEL = 1 << 20          # a label bit no inventory here sets: a group that needs it fits nowhere


def dom_level(island, level, level_size, parent):
    """int64[N]: the level-`level` domain of every node, -1 for none (plain Python, one step up per level)."""
    off = TC.offsets(level_size)
    par = [] if parent is None else [int(x) for x in parent]
    out = []
    for isl in np.asarray(island).reshape(-1):
        d = int(isl) if 0 <= int(isl) < int(level_size[0]) else -1
        for l in range(level):
            if d >= 0:
                d = par[off[l] + d]
        out.append(d)
    return np.array(out, dtype=np.int64)


def pod_offsets(group_count):
    off = [0]
    for c in group_count:
        off.append(off[-1] + max(0, int(c)))
    return off


def place(res, labels, island, batch, job_domain, level, level_size, parent):
    """(pod_node int32[P], job_status int32[J], residual_after int64[4][N]) by the C oracle, domain by domain."""
    res = np.array(res, dtype=np.int64, copy=True)
    labels = np.asarray(labels, dtype=np.uint32)
    dom = dom_level(island, level, level_size, parent)
    jgo = [int(x) for x in batch.job_group_off]
    J = len(jgo) - 1
    job_domain = np.asarray(job_domain, dtype=np.int64).reshape(-1)
    assert job_domain.shape == (J,) and ((job_domain >= 0) & (job_domain < level_size[level])).all()
    poff = pod_offsets(batch.group_count)
    pods = np.full(poff[-1], -1, dtype=np.int32)
    status = np.zeros(J, dtype=np.int32)
    for d in np.unique(job_domain):
        nodes = np.nonzero(dom == d)[0]                     # ascending global ids
        jobs = np.nonzero(job_domain == d)[0]               # ascending: the oracle orders them by priority itself
        groups = [g for j in jobs for g in range(jgo[j], jgo[j + 1])]
        sub_off = np.cumsum([0] + [jgo[j + 1] - jgo[j] for j in jobs]).astype(np.int32)
        if len(nodes) == 0:                                 # no node: a job fails iff it has a pod to place
            for j in jobs:
                status[j] = int(any(int(batch.group_count[g]) > 0 for g in range(jgo[j], jgo[j + 1])))
            continue
        g_idx = np.array(groups, dtype=np.int64)
        sp, ss, sr = oracle.place_greedy(res[:, nodes], labels[nodes], sub_off, np.asarray(batch.priority)[jobs],
                                         np.asarray(batch.group_count)[g_idx] if len(groups) else np.zeros(0, np.int32),
                                         np.asarray(batch.group_req).reshape(-1, 4)[g_idx] if len(groups) else np.zeros((0, 4), np.int64),
                                         np.asarray(batch.group_need)[g_idx] if len(groups) else np.zeros(0, np.uint32))
        res[:, nodes] = sr
        status[jobs] = ss
        at = 0
        for g in groups:                                    # the sub-batch's pod slots are its groups' in order
            c = max(0, int(batch.group_count[g]))
            local = sp[at:at + c]
            pods[poff[g]:poff[g] + c] = np.where(local >= 0, nodes[np.clip(local, 0, None)], -1)
            at += c
    return pods, status, res


def place_python(res, labels, island, batch, job_domain, level, level_size, parent):
    """The same answer by semantics.place_greedy_appendix_b's loop with the domain condition added to the fit.
    Returns (pods list, status list, residual [4][N] lists, rollbacks): rollbacks = [(job, nodes its pods had
    taken before it failed, in placement order)]."""
    R = [[int(x) for x in row] for row in res]
    dom = dom_level(island, level, level_size, parent)
    members = {}
    for n, d in enumerate(dom):
        members.setdefault(int(d), []).append(n)
    J = len(batch.priority)
    poff = pod_offsets(batch.group_count)
    pods = [-1] * poff[-1]
    status = [0] * J
    rollbacks = []

    def argmin(cands, q, need):
        best = None
        for n in cands:                                     # fit: the node is in the job's domain, and Appendix B's
            k = S.appendix_b_key([R[d][n] for d in range(4)], int(labels[n]), q, need, n)
            if k is not None and (best is None or k < best):
                best = k
        return best

    for j in sorted(range(J), key=lambda j: (-int(batch.priority[j]), j)):
        cands = members.get(int(job_domain[j]), [])
        placed, ok = [], True
        for g in range(int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])):
            q = [int(x) for x in batch.group_req[g]]
            need, c = int(batch.group_need[g]), int(batch.group_count[g])
            if need & ISLAND and c > 0:
                qe = [x * c for x in q]
                best = argmin(cands, qe, need) if all(v <= S.INT64_MAX for v in qe) else None
                if best is None:
                    ok = False
                    break
                n = best & 0xFFFFFF
                for p in range(c):
                    for d in range(4):
                        R[d][n] -= q[d]
                    pods[poff[g] + p] = n
                    placed.append((g, p, n))
                continue
            for p in range(c):
                best = argmin(cands, q, need)
                if best is None:
                    ok = False
                    break
                n = best & 0xFFFFFF
                for d in range(4):
                    R[d][n] -= q[d]
                pods[poff[g] + p] = n
                placed.append((g, p, n))
            if not ok:
                break
        if not ok:
            for g, p, n in placed:
                for d in range(4):
                    R[d][n] += int(batch.group_req[g][d])
                pods[poff[g] + p] = -1
            status[j] = 1
            rollbacks.append((j, [n for _, _, n in placed]))
    return pods, status, R, rollbacks


def case_conditions(batch, job_domain, pods, status, rollbacks):
    """What a named case must show, on the checker's own answer: (some job placed, some job unschedulable, some
    unschedulable job had taken pods on two or more nodes -- a real rollback --, some lower-priority job of the same
    domain was placed on nodes such a rollback gave back)."""
    poff = pod_offsets(batch.group_count)
    real = [(j, set(nodes)) for j, nodes in rollbacks if len(set(nodes)) >= 2]
    reused = False
    for j, nodes in real:
        for k in range(len(status)):
            if status[k] == 0 and int(job_domain[k]) == int(job_domain[j]) and int(batch.priority[k]) < int(batch.priority[j]):
                mine = set(int(x) for x in pods[poff[int(batch.job_group_off[k])]:poff[int(batch.job_group_off[k + 1])]])
                reused |= bool(mine & nodes)
    return (any(s == 0 for s in status), any(s == 1 for s in status), bool(real), reused)


# ---------------------------------------------------------------- shared inputs

@dataclass
class Case:
    cap: np.ndarray
    used: np.ndarray
    labels: np.ndarray        # the engine's labels
    island: np.ndarray
    level_size: list
    parent: object
    level: int
    batch: synth.JobBatch
    job_domain: np.ndarray

    def residual(self):
        return self.cap - self.used


def make_batch(jobs):
    """JobBatch and job_domain of [(domain, priority, [(count, request[4], need), ...]), ...]."""
    off, pri, cnt, req, need, dom = [0], [], [], [], [], []
    for d, p, groups in jobs:
        for c, q, nd in groups:
            cnt.append(c)
            req.append(q)
            need.append(nd)
        off.append(len(cnt))
        pri.append(p)
        dom.append(d)
    return (synth.JobBatch(np.array(off, dtype=np.int32), np.array(pri, dtype=np.int32), np.array(cnt, dtype=np.int32),
                           np.array(req, dtype=np.int64).reshape(-1, 4), np.array(need, dtype=np.uint32),
                           np.zeros(len(pri), dtype=np.int8)),
            np.array(dom, dtype=np.int32))


_CPU = [500, 2000, 8000, 16000]
_MEM = [1 * GiB, 4 * GiB, 16 * GiB, 64 * GiB]
_EPH = [0, 0, 10 * GiB, 50 * GiB]


def job_mix(res, labels, island, level, level_size, parent, seed, max_domains=10):
    """A job mix for the hierarchy's `level`: multi-group jobs, island groups, zero-count groups, zero requests,
    equal priorities, several jobs per domain with mixed priorities, a job whose domain is empty (where the level
    has one) and -- in the domain with the most usable nodes, where one has two -- a job that takes pods on two
    nodes and then fails, followed by a lower-priority job that fits what it gave back."""
    rng = np.random.default_rng(seed)
    dom = dom_level(island, level, level_size, parent)
    n_dom = int(level_size[level])
    size = np.bincount(dom[dom >= 0], minlength=n_dom)
    jobs = []

    def group():
        kind = int(rng.integers(0, 10))
        q = [int(rng.choice(_CPU)), int(rng.choice(_MEM)), int(rng.integers(0, 3) == 0), int(rng.choice(_EPH))]
        if kind == 0:
            return (int(rng.integers(1, 5)), [0, 0, 0, 0], 0)               # a zero request
        if kind == 1:
            return (0, q, 0)                                                # a zero-count group
        if kind == 2:
            return (int(rng.integers(1, 4)), q, ISLAND | (1 if q[2] else 0))    # an island group
        if kind == 3:
            return (0, q, ISLAND)                                           # an island group without pods
        return (int(rng.integers(1, 7)), q, 1 if q[2] else 0)

    populated = np.nonzero(size > 0)[0]
    chosen = list(rng.permutation(populated)[:max_domains])
    for d in chosen:
        for _ in range(int(rng.integers(2, 5))):                            # several jobs per domain
            jobs.append((int(d), int(rng.choice([0, 1, 1, 5])), [group() for _ in range(int(rng.integers(1, 4)))]))
    if chosen:                                                              # every ingredient at least once
        d0 = int(chosen[0])
        jobs.append((d0, 1, []))                                            # a job without groups
        jobs.append((d0, 1, [(3, [0, 0, 0, 0], 0), (0, [500, GiB, 0, 0], 0)]))          # zero request, zero count
        jobs.append((d0, 1, [(2, [500, GiB, 0, 0], ISLAND), (1, [500, GiB, 0, 0], 0)]))   # an island group first
        jobs.append((d0, 5, [(1, [2000, GiB, 0, 0], 0)]))                   # the same domain, another priority
    empty = np.nonzero(size == 0)[0]
    if len(empty):
        jobs.append((int(empty[0]), 3, [(2, [500, GiB, 0, 0], 0)]))         # a domain without nodes: unschedulable
        jobs.append((int(empty[0]), 3, [(0, [500, GiB, 0, 0], 0)]))         # ... but a job without pods is placed
    # the rollback pair: in the domain with the most nodes whose residuals are all >= 0 and whose cpu is > 0
    res = np.asarray(res)
    usable = (res >= 0).all(axis=0) & (res[0] > 0) & (dom >= 0)
    per = np.bincount(dom[usable], minlength=n_dom)
    if per.max(initial=0) >= 2:
        d = int(per.argmax())
        cpus = np.sort(res[0][usable & (dom == d)])
        rb = int(cpus[-2])          # the second largest cpu residual: two nodes hold such a pod, and the largest
        c = int(cpus[-1]) // rb + 1   # holds one pod fewer than this, so the pods land on two nodes at least
        jobs.append((d, 100, [(c, [rb, 0, 0, 0], 0), (1, [1, 0, 0, 0], NO_LABEL)]))   # two nodes, then no fit
        jobs.append((d, 99, [(1, [rb, 0, 0, 0], 0)]))                                  # takes what came back
    order = rng.permutation(len(jobs))
    return make_batch([jobs[i] for i in order])


def tree_case(name, n, level, seed=31):
    """A named hierarchy (tree_capacity.tree) over the synth inventory of n nodes, with a job mix for `level`."""
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    batch, job_domain = job_mix(cap - used, labels, island, level, level_size, parent, seed + 7 * level + n)
    return Case(cap, used, labels, island, list(level_size), parent, level, batch, job_domain)


def tree_levels(name, n):
    return range(len(TC.tree(name, n)[1]))


def max_domain_nodes(case):
    dom = dom_level(case.island, case.level, case.level_size, case.parent)
    return int(np.bincount(dom[dom >= 0], minlength=1).max())


def one_level_case(sizes, jobs, seed=41, pad=3):
    """One level whose domain k has sizes[k] nodes, dealt in a shuffled order over the inventory (plus `pad` nodes
    in no domain); jobs as for make_batch."""
    ids = np.concatenate([np.full(s, k, dtype=np.int32) for k, s in enumerate(sizes)] + [np.full(pad, -1, dtype=np.int32)])
    rng = np.random.default_rng(seed)
    rng.shuffle(ids)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(len(ids), seed), ids)
    batch, job_domain = make_batch(jobs)
    return Case(cap, used, labels, island, [len(sizes)], None, 0, batch, job_domain)


def check_engine(eng, case, load=True):
    """Load the case (unless the engine already holds it), run the call and compare pods, statuses and residuals
    with the checker, cell by cell.  Returns the checker's (pods, status, residual)."""
    if load:
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before = eng.read_residuals()
    want = place(before, case.labels, case.island, case.batch, case.job_domain, case.level, case.level_size, case.parent)
    b = case.batch
    pods, st = eng.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                        case.job_domain, case.level, case.level_size, case.parent)
    assert np.array_equal(st, want[1]), (st.tolist(), want[1].tolist())
    assert np.array_equal(pods, want[0])
    assert np.array_equal(eng.read_residuals(), want[2])
    return want
