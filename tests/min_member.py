"""Checker for pe_place_min_member_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): pe_place_greedy_domains' with every job in two phases.  M_j = the job's pod
total T_j for min_member -1 (or no min_member), else min_member[j]; group g's mandatory pods are
m_g = clamp(M_j - pods of the job's earlier groups, 0, count_g), an island group with m_g > 0 being mandatory as a
whole; o_g = count_g - m_g are optional.  Phase 1 places the mandatory pods all-or-nothing; phase 2, after a
placed phase 1, places every group's optional pods until one finds no node (an optional island group: its one
unit or nothing) and rolls nothing back.  Two independent statements of it:

    place_python(...)  domain_placement.place_python's loop, one pod at a time in Python integers
    place(...)         through the C oracle, job by job on the sub-inventory of the job's domain: phase 1 is
                       oracle.place_greedy with the single job at the counts m_g; an optional group without the
                       island flag is a batch of o_g one-pod jobs of equal priority (each placed or not on its
                       own, in index order); an optional island group is one job

`labels` are the engine's labels: synth.island_labels applied.
"""
from dataclasses import dataclass

import numpy as np

import domain_capacity as DC
import domain_placement as DP
import tree_capacity as TC
import oracle
from oracle import semantics as S
from placement import synth

GiB = DP.GiB
ISLAND = DP.ISLAND
NO_LABEL = DP.NO_LABEL
ALL = -1                    # PE_MIN_MEMBER_ALL
Q = [16000, 64 * GiB, 0, 0]
Q_GPU = [8000, 32 * GiB, 2, 50 * GiB]
ONE = [1, 0, 0, 0]          # one millicpu


def shares(batch, min_member):
    """(m, o, M, T): per group the mandatory and optional pods, per job M_j and T_j, in Python integers."""
    jgo = [int(x) for x in batch.job_group_off]
    J = len(jgo) - 1
    cnt = [max(0, int(c)) for c in batch.group_count]
    m, o, Ms, Ts = [0] * len(cnt), [0] * len(cnt), [], []
    for j in range(J):
        T = sum(cnt[jgo[j]:jgo[j + 1]])
        mm = ALL if min_member is None else int(min_member[j])
        assert -1 <= mm <= T, (j, mm, T)
        M = T if mm == ALL else mm
        before = 0
        for g in range(jgo[j], jgo[j + 1]):
            mg = min(max(M - before, 0), cnt[g])
            if mg > 0 and int(batch.group_need[g]) & ISLAND:
                mg = cnt[g]
            m[g], o[g] = mg, cnt[g] - mg
            before += cnt[g]
        Ms.append(M)
        Ts.append(T)
    return m, o, Ms, Ts


def job_order(batch):
    return sorted(range(len(batch.priority)), key=lambda j: (-int(batch.priority[j]), j))


def place(res, labels, island, batch, min_member, job_domain, level, level_size, parent):
    """(pod_node int32[P], job_status int32[J], group_pods int32[G], residual_after int64[4][N]) by the C oracle."""
    res = np.array(res, dtype=np.int64, copy=True)
    labels = np.asarray(labels, dtype=np.uint32)
    dom = DP.dom_level(island, level, level_size, parent)
    jgo = [int(x) for x in batch.job_group_off]
    J = len(jgo) - 1
    m, o, _, _ = shares(batch, min_member)
    req = np.asarray(batch.group_req, dtype=np.int64).reshape(-1, 4)
    need = np.asarray(batch.group_need, dtype=np.uint32)
    poff = DP.pod_offsets(batch.group_count)
    pods = np.full(poff[-1], -1, dtype=np.int32)
    status = np.zeros(J, dtype=np.int32)
    gp = np.zeros(len(m), dtype=np.int32)
    zero = np.zeros(1, dtype=np.int32)
    for j in job_order(batch):
        g0, g1 = jgo[j], jgo[j + 1]
        nodes = np.nonzero(dom == int(job_domain[j]))[0]     # ascending global ids keep the key order
        if len(nodes) == 0:                                  # no node: unschedulable iff a pod is mandatory
            status[j] = int(any(m[g] > 0 for g in range(g0, g1)))
            continue
        if g0 == g1:
            continue
        lab = labels[nodes]
        # phase 1: the job alone at its mandatory counts
        sp, ss, sr = oracle.place_greedy(res[:, nodes], lab, np.array([0, g1 - g0], dtype=np.int32), zero,
                                         np.array(m[g0:g1], dtype=np.int32), req[g0:g1], need[g0:g1])
        if int(ss[0]) != 0:
            status[j] = 1
            continue
        at = 0
        for g in range(g0, g1):
            pods[poff[g]:poff[g] + m[g]] = nodes[sp[at:at + m[g]]]
            at += m[g]
            gp[g] = m[g]
        # phase 2: group by group, nothing comes back
        for g in range(g0, g1):
            if o[g] == 0:
                continue
            if int(need[g]) & ISLAND:
                k_off, k_cnt, k = np.array([0, 1], dtype=np.int32), np.array([o[g]], dtype=np.int32), 1
            else:
                k = o[g]
                k_off, k_cnt = np.arange(k + 1, dtype=np.int32), np.ones(k, dtype=np.int32)
            sp, ss, sr = oracle.place_greedy(sr, lab, k_off, np.zeros(k, dtype=np.int32), k_cnt,
                                             np.repeat(req[g:g + 1], k, axis=0), np.repeat(need[g:g + 1], k))
            ok = ss == 0
            got = int(ok.sum()) * int(k_cnt[0])
            assert ok[:int(ok.sum())].all() and (sp[:got] >= 0).all() and (sp[got:] < 0).all()   # a prefix
            pods[poff[g] + m[g]:poff[g] + m[g] + got] = nodes[sp[:got]]
            gp[g] += got
        res[:, nodes] = sr
    return pods, status, gp, res


def place_python(res, labels, island, batch, min_member, job_domain, level, level_size, parent):
    """The same answer pod by pod in Python integers.  Returns (pods list, status list, group_pods list, residual
    [4][N] lists, rollbacks): rollbacks = [(job, nodes its pods had taken before it failed, in placement order)]."""
    R = [[int(x) for x in row] for row in res]
    dom = DP.dom_level(island, level, level_size, parent)
    members = {}
    for n, d in enumerate(dom):
        members.setdefault(int(d), []).append(n)
    m, o, _, _ = shares(batch, min_member)
    J = len(batch.priority)
    poff = DP.pod_offsets(batch.group_count)
    pods = [-1] * poff[-1]
    status = [0] * J
    gp = [0] * len(m)
    rollbacks = []

    def argmin(cands, q, need):
        best = None
        for n in cands:
            k = S.appendix_b_key([R[d][n] for d in range(4)], int(labels[n]), q, need, n)
            if k is not None and (best is None or k < best):
                best = k
        return best

    def put(g, slot, n, q):
        for d in range(4):
            R[d][n] -= q[d]
        pods[poff[g] + slot] = n

    def run(cands, g, first, count, placed):
        """Pods [first, first + count) of group g, in order; how many found a node (an island group: all or none)."""
        q = [int(x) for x in batch.group_req[g]]
        need = int(batch.group_need[g])
        if need & ISLAND:
            qe = [x * count for x in q]
            best = argmin(cands, qe, need) if all(v <= S.INT64_MAX for v in qe) else None
            if best is None:
                return 0
            for p in range(count):
                put(g, first + p, best & 0xFFFFFF, q)
                placed.append((g, first + p, best & 0xFFFFFF))
            return count
        for p in range(count):
            best = argmin(cands, q, need)
            if best is None:
                return p
            put(g, first + p, best & 0xFFFFFF, q)
            placed.append((g, first + p, best & 0xFFFFFF))
        return count

    for j in job_order(batch):
        cands = members.get(int(job_domain[j]), [])
        groups = range(int(batch.job_group_off[j]), int(batch.job_group_off[j + 1]))
        placed, ok = [], True
        for g in groups:                                     # phase 1
            if m[g] > 0 and run(cands, g, 0, m[g], placed) < m[g]:
                ok = False
                break
        if not ok:
            for g, slot, n in placed:
                for d in range(4):
                    R[d][n] += int(batch.group_req[g][d])
                pods[poff[g] + slot] = -1
            status[j] = 1
            rollbacks.append((j, [n for _, _, n in placed]))
            continue
        for g in groups:                                     # phase 2
            gp[g] = m[g] + (run(cands, g, m[g], o[g], []) if o[g] > 0 else 0)
    return pods, status, gp, R, rollbacks


def conditions(batch, min_member, status, gp):
    """What every mix must show, on the checker's own answer: (a job placed in full, a job placed in part --
    0 < pods < T --, a job placed with optional pods of which none found a node, a failed job)."""
    _, o, _, T = shares(batch, min_member)
    jgo = [int(x) for x in batch.job_group_off]
    full = part = none = False
    for j in range(len(T)):
        if status[j] != 0:
            continue
        got = sum(int(gp[g]) for g in range(jgo[j], jgo[j + 1]))
        opt = sum(o[jgo[j]:jgo[j + 1]])
        full |= T[j] > 0 and got == T[j]
        part |= 0 < got < T[j]
        none |= opt > 0 and got == T[j] - opt
    return full, part, none, any(s == 1 for s in status)


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
    min_member: object        # int32 [J] or None

    def residual(self):
        return self.cap - self.used


def make_batch(jobs):
    """JobBatch, job_domain and min_member of [(domain, priority, min_member, [(count, request[4], need), ...]), ...]."""
    batch, dom = DP.make_batch([(d, p, groups) for d, p, _, groups in jobs])
    return batch, dom, np.array([mm for _, _, mm, _ in jobs], dtype=np.int32)


def draw_min_member(batch, rng):
    """min_member per job from {0, 1, a group edge, inside a group, T - 1, T, -1}, whatever of them the job has."""
    jgo = [int(x) for x in batch.job_group_off]
    out = []
    for j in range(len(jgo) - 1):
        cnt = [int(c) for c in batch.group_count[jgo[j]:jgo[j + 1]]]
        T = sum(cnt)
        edges = [sum(cnt[:k]) for k in range(1, len(cnt))]
        inside = [sum(cnt[:k]) + c // 2 for k, c in enumerate(cnt) if c >= 2]
        choice = [0, 1, T - 1, T, ALL] + edges[:1] + inside[:1] + inside[-1:]
        mm = int(choice[int(rng.integers(0, len(choice)))])
        out.append(min(max(mm, ALL), T))
    return out


def job_mix(res, labels, island, level, level_size, parent, seed, max_domains=10):
    """domain_placement.job_mix with a min_member per job, plus -- in the domain with the most usable nodes -- four
    jobs that run before all others and show, whatever the draw: a job placed in part (as many pods of the largest
    cpu residual as the domain holds, of 100 000), a job placed without any of its optional pods, a job placed in
    full, and a job whose last mandatory pod finds no node."""
    rng = np.random.default_rng(seed + 1000)
    base, dom = DP.job_mix(res, labels, island, level, level_size, parent, seed, max_domains)
    mm = draw_min_member(base, rng)
    jgo = [int(x) for x in base.job_group_off]
    jobs = [(int(dom[j]), int(base.priority[j]), mm[j],
             [(int(base.group_count[g]), [int(x) for x in base.group_req[g]], int(base.group_need[g]))
              for g in range(jgo[j], jgo[j + 1])]) for j in range(len(mm))]
    res = np.asarray(res)
    d_of = DP.dom_level(island, level, level_size, parent)
    usable = (res >= 0).all(axis=0) & (res[0] > 0) & (d_of >= 0)
    per = np.bincount(d_of[usable], minlength=int(level_size[level]))
    if per.max(initial=0) >= 1:
        d = int(per.argmax())
        top = int(res[0][usable & (d_of == d)].max())
        jobs.append((d, 400, 1, [(100000, [top, 0, 0, 0], 0)]))                       # in part
        jobs.append((d, 300, 1, [(1, ONE, 0), (2, ONE, NO_LABEL)]))                   # none of the optional pods
        jobs.append((d, 250, ALL, [(2, [0, 0, 0, 0], 0)]))                            # in full
        jobs.append((d, 200, 3, [(2, [0, 0, 0, 0], 0), (1, ONE, NO_LABEL), (5, ONE, 0)]))   # the third pod fails
    order = rng.permutation(len(jobs))
    return make_batch([jobs[i] for i in order])


def tree_case(name, n, level, seed=31):
    """A named hierarchy (tree_capacity.tree) over the synth inventory of n nodes, with a job mix for `level`."""
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    batch, dom, mm = job_mix(cap - used, labels, island, level, level_size, parent, seed + 7 * level + n)
    return Case(cap, used, labels, island, list(level_size), parent, level, batch, dom, mm)


def one_level_case(sizes, jobs, seed=41, pad=3):
    """One level whose domain k has sizes[k] nodes (domain_placement.one_level_case); jobs as for make_batch."""
    c = DP.one_level_case(sizes, [(d, p, groups) for d, p, _, groups in jobs], seed, pad)
    return Case(c.cap, c.used, c.labels, c.island, c.level_size, None, 0, c.batch, c.job_domain,
                np.array([mm for _, _, mm, _ in jobs], dtype=np.int32))


def size_case(size):
    """Domain 0 of `size` nodes and domain 1 of five: a job cut inside a group, one cut on a group edge, a job
    that takes nodes and is rolled back followed by one that reuses them, an island group on the cut (mandatory as
    a whole), optional groups that find no node, and the small domain with a job placed in part."""
    spread = min(4 * size, 300)      # pods that fill node after node
    jobs = [(0, 7, 2 + spread // 2, [(2, Q_GPU, 1), (spread, Q, 0), (3, ONE, 0)]),          # cut inside a group
            (0, 6, 3, [(3, Q, 0), (spread, Q, 0)]),                                         # cut on a group edge
            (0, 9, ALL, [(spread, Q, 0), (min(size, 40), [500, GiB, 0, 0], 0), (1, ONE, NO_LABEL)]),   # rolled back
            (0, 8, spread // 2, [(spread, Q, 0)]),                                          # on the nodes that came back
            (0, 11, 3, [(2, ONE, 0), (3, [500, GiB, 0, 0], ISLAND), (4, ONE, 0)]),          # an island group on the cut
            (0, 10, 1, [(1, ONE, 0), (2, ONE, NO_LABEL)]),                                  # none of the optional pods
            (0, 10, ALL, [(2, [0, 0, 0, 0], 0)]),
            (1, 0, 1, [(3, ONE, 0)]),                                                       # the second, small domain
            (1, 0, 2, [(1000, Q, 0)]),
            (0, 10, 0, [(2, ONE, NO_LABEL), (0, Q, 0), (2, ONE, 0)])]                       # no node holds it; the next places
    return one_level_case([size, 5], jobs, seed=size)


def all_active_case(n=2500):
    """Every rack of "racks32" active: two jobs per rack and a third in every fifth, cut at every kind of place."""
    island, level_size, parent = TC.tree("racks32", n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    jobs = []
    for d in range(level_size[0]):
        jobs.append((d, d % 3, d % 4, [(1 + d % 7, Q, 0), (d % 2, Q_GPU, 1), (2, ONE, NO_LABEL if d % 6 == 0 else 0)]))
        jobs.append((d, 1, [ALL, 0, 5][d % 3], [(3, ONE, 0), (2, ONE, NO_LABEL if d % 4 == 1 else 0)]))
    jobs += [(d, 1, 1, [(200, Q, 0)]) for d in range(0, level_size[0], 5)]
    batch, dom, mm = make_batch(jobs)
    return Case(cap, used, labels, island, list(level_size), parent, 0, batch, dom, mm)


# a rack of two nodes with 8 free GPUs each (the header's example); Master 1 x 2 GPUs, Workers 6 x 3 GPUs
RACK_CAP = np.array([[64000] * 2, [256 * GiB] * 2, [8] * 2, [0] * 2], dtype=np.int64)


def gpus(g):
    return [1000, GiB, g, 0]


def rack_case(min_member, jobs=None, cap=RACK_CAP, island=None, sizes=(1,)):
    n = cap.shape[1]
    jobs = jobs or [(0, 0, min_member, [(1, gpus(2), 0), (6, gpus(3), 0)])]
    batch, dom, mm = make_batch(jobs)
    island = np.zeros(n, dtype=np.int32) if island is None else np.asarray(island, dtype=np.int32)
    labels = synth.island_labels(np.ones(n, dtype=np.uint32), island)
    return Case(cap, np.zeros_like(cap), labels, island, list(sizes), None, 0, batch, dom, mm)


def node_cap(gpu):
    """One column per entry: plenty of cpu and memory, `gpu` free GPUs."""
    n = len(gpu)
    return np.array([[64000] * n, [256 * GiB] * n, list(gpu), [0] * n], dtype=np.int64)


def traps():
    """{name: (Case, status list, group_pods list)}: hand-made cases with the answer worked out by hand."""
    t = {}
    t["rack_min4"] = (rack_case(4), [0], [1, 4])
    t["rack_min6"] = (rack_case(6), [1], [0, 0])
    # the cut (M = 2) falls inside the island group of 3: mandatory as a whole, 1 + 3 x 2 GPUs on 8, then 1 of 2 optional
    t["island_cut"] = (rack_case(0, [(0, 0, 2, [(1, gpus(1), 0), (3, gpus(2), ISLAND), (2, gpus(1), 0)])],
                                 cap=node_cap([8])), [0], [1, 3, 1])
    # ... and on a node of 6 GPUs the whole island group does not fit: the job fails although 2 pods would
    t["island_cut_fails"] = (rack_case(0, [(0, 0, 2, [(1, gpus(1), 0), (3, gpus(2), ISLAND)])], cap=node_cap([6])),
                             [1], [0, 0])
    # optional island groups: 2 x 3 GPUs fit node 0 or 1 (8 free, 7 after the master), 3 x 3 fit no node
    t["island_optional"] = (rack_case(0, [(0, 0, 1, [(1, gpus(1), 0), (2, gpus(3), ISLAND), (3, gpus(3), ISLAND),
                                                     (1, gpus(1), 0)])]), [0], [1, 2, 0, 1])
    # an optional group whose need no node has, followed by a group that places
    t["need_then_places"] = (rack_case(0, [(0, 0, 0, [(2, gpus(1), NO_LABEL), (3, gpus(1), 0)])]), [0], [0, 3])
    # a failed job (needs 9 GPUs on one node at M = T) whose resources the next job of the domain takes
    t["failed_then_next"] = (rack_case(0, [(0, 5, ALL, [(2, gpus(7), 0), (1, gpus(9), 0)]),
                                           (0, 1, 2, [(2, gpus(8), 0), (1, gpus(1), 0)])]), [1, 0], [0, 0, 2, 0])
    # the same job fails at T (5 x 4 GPUs on 2 x 8) and is placed at T - 1
    t["fails_at_T"] = (rack_case(0, [(0, 0, 5, [(5, gpus(4), 0)])]), [1], [0])
    t["placed_at_T_minus_1"] = (rack_case(0, [(0, 0, 4, [(5, gpus(4), 0)])]), [0], [4])
    # zero-count groups on either side of the cut
    t["zero_counts"] = (rack_case(0, [(0, 0, 2, [(0, gpus(9), 0), (2, gpus(4), 0), (0, gpus(9), ISLAND), (0, gpus(1), 0),
                                                 (3, gpus(4), 0)])]), [0], [0, 2, 0, 0, 2])
    # a domain without nodes (domain 1 of 2): M = 0 is placed with 0 pods, M = 1 is unschedulable; no groups: placed
    t["empty_domain"] = (rack_case(0, [(1, 0, 0, [(2, gpus(1), 0)]), (1, 0, 1, [(2, gpus(1), 0)]), (1, 0, ALL, []),
                                       (1, 0, 0, [(0, gpus(1), 0)])], sizes=(2,)), [0, 1, 0, 0], [0, 0, 0])
    return t


def check_engine(eng, case, load=True):
    """Load the case (unless the engine already holds it), run the call and compare every pod slot, status, group
    count, job count and residual cell with the checker.  Returns the checker's (pods, status, group_pods, residual)."""
    if load:
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before = eng.read_residuals()
    want = place(before, case.labels, case.island, case.batch, case.min_member, case.job_domain, case.level,
                 case.level_size, case.parent)
    b = case.batch
    pods, st, gp, jp = eng.place_min_member_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                                    case.min_member, case.job_domain, case.level, case.level_size,
                                                    case.parent)
    assert np.array_equal(st, want[1]), (st.tolist(), want[1].tolist())
    assert np.array_equal(gp, want[2]), (gp.tolist(), want[2].tolist())
    assert np.array_equal(pods, want[0])
    jgo = np.asarray(b.job_group_off, dtype=np.int64)
    assert jp.dtype == np.int64 and jp.tolist() == [int(want[2][jgo[j]:jgo[j + 1]].sum()) for j in range(len(st))]
    assert np.array_equal(eng.read_residuals(), want[3])
    return want
