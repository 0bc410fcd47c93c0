"""Checker for pe_gang_preempt_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): pair p comes with an ordered list of candidate victims.  A JUDGEMENT asks whether
pe_place_greedy_domains would place the pair's job alone in the pair's domain against R(E): the current residuals
with every pod that the victims at the list positions E hold on a node of the domain given back.  Phase 1 walks the
prefixes in ascending order to the first that is placed; phase 2 puts back, from position prefix - 2 down to 0,
every victim the job is placed without.

    two_phase(judge, K)   the procedure, stated once over a judgement function judge(E) -> bool
    judge_oracle          gang_fit.placed_alone: the C oracle on the domain's sub-inventory of an adjusted copy of
                          the residuals
    judge_python          gang_fit.fit_python: one pod at a time in plain Python integers

`labels` are the engine's labels: synth.island_labels applied.
"""
from dataclasses import dataclass

import numpy as np

import domain_placement as DP
import gang_fit as GF
from placement import synth

GiB = DP.GiB
ISLAND = DP.ISLAND
MAX_LIST = 64               # PE_MAX_PAIR_VICTIMS


@dataclass
class Victims:
    """Placed gangs in the shape the placement calls take and return."""
    group_off: np.ndarray      # int32 [V + 1]
    group_count: np.ndarray    # int32 [VG]
    group_req: np.ndarray      # int64 [VG][4]
    pod_node: np.ndarray       # int32 [sum of counts]: global node id per pod slot, -1 = skipped
    priority: np.ndarray       # int32 [V]: what the generator orders the lists by; the engine never sees it

    def __len__(self):
        return len(self.group_off) - 1

    def arrays(self):
        return self.group_off, self.group_count, self.group_req, self.pod_node

    def pods(self, v):
        """[(node, request[4]), ...] of victim v's pod slots that hold a node."""
        out = []
        at = int(np.clip(self.group_count[:int(self.group_off[v])], 0, None).sum())
        for g in range(int(self.group_off[v]), int(self.group_off[v + 1])):
            for _ in range(int(self.group_count[g])):
                if int(self.pod_node[at]) >= 0:
                    out.append((int(self.pod_node[at]), [int(x) for x in self.group_req[g]]))
                at += 1
        return out


def make_victims(vics):
    """Victims of [(priority, [(request[4], [node per pod slot]), ...]), ...]."""
    off, cnt, req, pods, pri = [0], [], [], [], []
    for p, groups in vics:
        for q, nodes in groups:
            cnt.append(len(nodes))
            req.append(q)
            pods.extend(nodes)
        off.append(len(cnt))
        pri.append(p)
    return Victims(np.array(off, dtype=np.int32), np.array(cnt, dtype=np.int32), np.array(req, dtype=np.int64).reshape(-1, 4),
                   np.array(pods, dtype=np.int32), np.array(pri, dtype=np.int32))


# ---------------------------------------------------------------- the rule

def two_phase(judge, K):
    """(prefix, mask, count) of one pair with K candidates; judge(E) for a sorted tuple E of list positions."""
    prefix = next((k for k in range(K + 1) if judge(tuple(range(k)))), -1)
    if prefix < 0:
        return -1, 0, -1
    E = list(range(prefix))
    for i in range(prefix - 2, -1, -1):
        without = [x for x in E if x != i]
        if judge(tuple(without)):
            E = without
    return prefix, sum(1 << i for i in E), len(E)


def released(res, dom, domain, pods_of, victims):
    """R(E): a copy of res with every pod of `victims` on a node of `domain` given back."""
    out = np.array(res, dtype=np.int64, copy=True)
    for v in victims:
        for n, q in pods_of[v]:
            if int(dom[n]) == domain:
                out[:, n] += np.array(q, dtype=np.int64)
    return out


def judge_oracle(res, labels, nodes, groups):
    return GF.placed_alone(res, labels, nodes, groups)


def judge_python(res, labels, nodes, groups):
    return GF.fit_python(res, labels, nodes, groups)[0] == 1


def answers(res, labels, island, batch, vic, pair_job, pair_domain, pair_vic_off, pair_vic, level, level_size, parent,
            judge=judge_oracle, counts=None):
    """(prefix int32[P], victims uint64[P], count int32[P], best int32[J]) by two_phase over `judge`.  counts: a
    list that receives the judgements made per pair."""
    dom = DP.dom_level(island, level, level_size, parent)
    members = GF.members_of(island, level, level_size, parent)
    none = np.zeros(0, dtype=np.int64)
    pods_of = [vic.pods(v) for v in range(len(vic))]
    P = len(pair_job)
    prefix, mask, count = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.int32)
    memo = {}
    for p in range(P):
        j, d = int(pair_job[p]), int(pair_domain[p])
        lst = tuple(int(v) for v in pair_vic[int(pair_vic_off[p]):int(pair_vic_off[p + 1])])
        assert len(lst) <= MAX_LIST and len(set(lst)) == len(lst)
        if (j, d, lst) not in memo:
            groups, nodes, made = GF.job_groups(batch, j), members.get(d, none), [0]

            def one(E):
                made[0] += 1
                return judge(released(res, dom, d, pods_of, [lst[i] for i in E]), labels, nodes, groups)
            memo[j, d, lst] = two_phase(one, len(lst)) + (made[0],)
        prefix[p], mask[p], count[p], made = memo[j, d, lst]
        assert made <= len(lst) + 1 + max(0, int(prefix[p]) - 1)
        if counts is not None:
            counts.append(made)
    return prefix, mask, count, best_of(pair_job, count, len(batch.job_group_off) - 1)


def best_of(pair_job, count, J):
    """int32[J]: the pair of job j with the smallest count >= 0, ties to the smallest p; -1 when there is none."""
    best = np.full(J, -1, dtype=np.int32)
    for p in range(len(pair_job) - 1, -1, -1):
        j = int(pair_job[p])
        if count[p] >= 0 and (best[j] < 0 or count[p] <= count[best[j]]):
            best[j] = p
    return best


def final_set(pair_vic_off, pair_vic, p, mask):
    """The victims of pair p's list at the positions of `mask`."""
    lst = pair_vic[int(pair_vic_off[p]):int(pair_vic_off[p + 1])]
    return [int(lst[i]) for i in range(len(lst)) if int(mask) >> i & 1]


def used_without(case, vic, victims, domain):
    """case.used with the pods of `victims` on the nodes of `domain` released: what a fresh engine is loaded with to
    see R(E) as its current residuals."""
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    used = np.array(case.used, dtype=np.int64, copy=True)
    for v in victims:
        for n, q in vic.pods(v):
            if int(dom[n]) == domain:
                used[:, n] -= np.array(q, dtype=np.int64)
    return used


# ---------------------------------------------------------------- shared inputs

@dataclass
class PCase:
    case: DP.Case              # the inventory with the victims accounted in `used`, the incoming batch and its level
    vic: Victims
    pair_job: np.ndarray
    pair_domain: np.ndarray
    pair_vic_off: np.ndarray
    pair_vic: np.ndarray

    def call_args(self):
        c, b = self.case, self.case.batch
        return (b.job_group_off, b.group_count, b.group_req, b.group_need) + self.vic.arrays() + \
            (self.pair_job, self.pair_domain, self.pair_vic_off, self.pair_vic, c.level, c.level_size, c.parent)

    def answers(self, res=None, judge=judge_oracle, counts=None):
        c = self.case
        return answers(c.residual() if res is None else res, c.labels, c.island, c.batch, self.vic, self.pair_job,
                       self.pair_domain, self.pair_vic_off, self.pair_vic, c.level, c.level_size, c.parent, judge, counts)


def fillers(res, case, n_domains=4):
    """Per domain, for the `n_domains` domains with the most nodes: a gang of one-pod-per-node cpu requests that
    takes every node with more than half of the domain's largest free cpu -- after it no node of the domain holds
    another pod of that request, however large the domain is.  Returns (jobs as for make_batch, {domain: request})."""
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    usable = (res >= 0).all(axis=0) & (dom >= 0)
    size = np.bincount(dom[usable], minlength=int(case.level_size[case.level]))
    jobs, ask = [], {}
    for d in np.argsort(-size, kind="stable")[:n_domains]:
        mine = usable & (dom == d)
        if not mine.any() or int(res[0][mine].max()) < 2:
            continue
        c = int(res[0][mine].max()) // 2 + 1                # a node holds one such pod at most
        jobs.append((int(d), 60, [(int((res[0][mine] >= c).sum()), [c, 0, 0, 0], 0)]))
        ask[int(d)] = c
    return jobs, ask


def resident_victims(case, rounds=16, want=MAX_LIST + 2):
    """Place the fillers, then the case's own job mix (and further mixes on what remains, until `want` gangs are placed
    or `rounds` mixes are spent) on the CPU with domain_placement.place.  The placed jobs that hold a pod are the
    victims: their groups and pod slots exactly as the placement returned them.  Returns (Victims, the residuals that
    remain, {domain: the cpu request no node of it holds any more})."""
    res = case.residual()
    vics = []
    fill, ask = fillers(res, case)
    batch, job_domain = DP.make_batch(fill)
    held = {}
    for r in range(-1, rounds):
        pods, status, res = DP.place(res, case.labels, case.island, batch, job_domain, case.level, case.level_size, case.parent)
        poff = DP.pod_offsets(batch.group_count)
        for j in np.nonzero(status == 0)[0]:
            g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
            if poff[g1] == poff[g0]:
                continue                                    # no pod: nothing to evict
            vics.append((int(batch.priority[j]), [([int(x) for x in batch.group_req[g]], pods[poff[g]:poff[g + 1]].tolist())
                                                  for g in range(g0, g1)]))
            if r < 0:
                held[int(job_domain[j])] = ask[int(job_domain[j])]
        if r >= 0 and len(vics) >= want:
            break
        batch, job_domain = (case.batch, case.job_domain) if r < 0 else \
            DP.job_mix(res, case.labels, case.island, case.level, case.level_size, case.parent, 977 + 13 * r)
    return make_victims(vics), res, held


def incoming_mix(res, case, vic, held, seed):
    """The incoming jobs: a second job mix sized against the residuals that remain; per filled domain a job of one pod
    of the request the filler left no room for (it needs an eviction); and per domain that holds two victims' pods
    on one node a job of one pod that asks for what that node has free plus what the LAST of them (in list order)
    holds there -- the fill-back returns whoever was released before."""
    batch, job_domain = DP.job_mix(res, case.labels, case.island, case.level, case.level_size, case.parent, seed)
    jobs = [(int(job_domain[j]), int(batch.priority[j]), GF.job_groups(batch, j)) for j in range(len(job_domain))]
    jobs += [(d, 50, [(1, [c, 0, 0, 0], 0)]) for d, c in sorted(held.items())]
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    order = list_order(vic)
    rank = {v: i for i, v in enumerate(order)}
    on = {}                                                 # node -> {victim: cpu it holds there}
    for v in range(len(vic)):
        for n, q in vic.pods(v):
            if q[0] > 0 and dom[n] >= 0:
                on.setdefault(n, {}).setdefault(v, 0)
                on[n][v] += q[0]
    extra = {}
    for n, hold in sorted(on.items()):
        if len(hold) >= 2 and int(dom[n]) not in extra and res[0][n] >= 0:
            last = max(hold, key=lambda v: rank[v])
            extra[int(dom[n])] = (int(dom[n]), 50, [(1, [int(res[0][n]) + hold[last], 0, 0, 0], 0)])
    jobs += list(extra.values())[:6]
    return DP.make_batch(jobs)


def list_order(vic):
    """The victims in eviction order: ascending priority, ties by index."""
    return sorted(range(len(vic)), key=lambda v: (int(vic.priority[v]), v))


def pair_lists(case, vic, pair_job, pair_domain, seed):
    """(pair_vic_off, pair_vic): per pair one victim that has no pod in the pair's domain (where there is one), then
    the victims that have a pod there, in ascending priority.  Where the victims allow it, the first pairs' lists
    are cut or padded with further strangers to the lengths 0, 1, 2, 63 and 64."""
    rng = np.random.default_rng(seed)
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    order = list_order(vic)
    inside = {}
    for v in order:
        for d in {int(dom[n]) for n, _ in vic.pods(v)}:
            inside.setdefault(d, []).append(v)
    forced = [0, 1, 2, MAX_LIST - 1, MAX_LIST]
    off, lists = [0], []
    for p in range(len(pair_job)):
        mine = list(inside.get(int(pair_domain[p]), []))[:MAX_LIST - 1]
        strangers = [v for v in rng.permutation(len(vic)).tolist() if v not in mine]
        lst = strangers[:1] + mine
        if p < len(forced) and forced[p] <= len(vic):
            lst = (lst + strangers[1:])[:forced[p]]
        lists += lst
        off.append(len(lists))
    return np.array(off, dtype=np.int32), np.array(lists, dtype=np.int32)


def tree_pcase(name, n, level, seed=71):
    """A named hierarchy with resident victims accounted in `used`, an incoming mix, pairs (gang_fit.pair_mix) and
    their candidate lists."""
    base = DP.tree_case(name, n, level)
    vic, res, held = resident_victims(base)
    used = base.cap - res                                   # raised by what the victims took
    batch, job_domain = incoming_mix(res, base, vic, held, seed + 5 * level + n)
    case = DP.Case(base.cap, used, base.labels, base.island, base.level_size, base.parent, level, batch, job_domain)
    pj, pd = GF.pair_mix(case, seed + 3 * level + n)
    pvo, pv = pair_lists(case, vic, pj, pd, seed + n)
    return PCase(case, vic, pj, pd, pvo, pv)


def one_level_pcase(sizes, seed=43):
    """One level whose domain k has sizes[k] nodes (domain 0 the contested one), with resident victims, an incoming
    mix and every job paired with domain 0, domain 1 and its own."""
    n_jobs = [(0, int(p), [(3, [2000, 4 * GiB, 0, 0], 0), (2, [500, GiB, 1, 0], 1)]) for p in range(4)] + \
             [(0, 2, [(2, [8000, 16 * GiB, 0, 0], ISLAND)]), (1, 1, [(1, [500, GiB, 0, 0], 0)])]
    base = DP.one_level_case(sizes, n_jobs, seed)
    vic, res, held = resident_victims(base, rounds=2, want=6)
    used = base.cap - res
    batch, job_domain = incoming_mix(res, base, vic, held, seed)
    case = DP.Case(base.cap, used, base.labels, base.island, base.level_size, base.parent, 0, batch, job_domain)
    J = len(job_domain)
    pj = np.repeat(np.arange(J, dtype=np.int32), 3)
    pd = np.stack([np.zeros(J), np.ones(J), job_domain], axis=1).astype(np.int32).reshape(-1)
    pvo, pv = pair_lists(case, vic, pj, pd, seed)
    return PCase(case, vic, pj, pd, pvo, pv)


# ---------------------------------------------------------------- the hand-made traps

def _inventory(res, island):
    """A Case skeleton of free nodes with residuals res [4][N] (cap = res + used, used filled in by the trap)."""
    island = np.array(island, dtype=np.int32)
    labels = synth.island_labels(np.ones(len(island), dtype=np.uint32), island)
    return np.array(res, dtype=np.int64), labels, island


def _trap(res, island, n_domains, vics, jobs, pairs):
    """res: the residuals with the victims in place; vics as make_victims; jobs as domain_placement.make_batch;
    pairs [(job, domain, [victims])]."""
    res, labels, island = _inventory(res, island)
    vic = make_victims(vics)
    used = np.zeros_like(res)
    for v in range(len(vic)):
        for n, q in vic.pods(v):
            used[:, n] += np.array(q, dtype=np.int64)
    batch, job_domain = DP.make_batch(jobs)
    case = DP.Case(res + used, used, labels, island, [n_domains], None, 0, batch, job_domain)
    off = np.cumsum([0] + [len(l) for _, _, l in pairs]).astype(np.int32)
    return PCase(case, vic, np.array([j for j, _, _ in pairs], dtype=np.int32), np.array([d for _, d, _ in pairs], dtype=np.int32),
                 off, np.array([v for _, _, l in pairs for v in l], dtype=np.int32))


def gpus(g, cpu=0, mem=0):
    return [cpu, mem, g, 0]


def trap_non_monotone():
    """The header's example: with X released A still takes n0 and B takes n1; with X and Y released A's smallest key
    is n1 and B fits nowhere.  The prefixes fit as no, yes, no.  Expected prefix 1, mask 0b01, count 1."""
    pc = _trap([[2000, 64000], [64 * GiB, 64 * GiB], [6, 4], [0, 0]], [0, 0], 1,
               [(0, [(gpus(5), [1])]), (1, [(gpus(4), [0])])],
               [(0, 9, [(1, gpus(5, 1000, GiB), 0), (1, gpus(5, 32000, GiB), 0)])],
               [(0, 0, [0, 1])])
    return pc, ([1], [0b01], [1], [0])


def trap_fill_back():
    """One node, 0 GPUs free of 8; victims X = 2, Y = 1, Z = 4 GPUs in that order; the job is 1 x 4 GPUs.  All three
    must go before it fits (2 + 1 < 4), then Y and X come back: prefix 3, mask 0b100, count 1."""
    pc = _trap([[64000], [64 * GiB], [0], [0]], [0], 1,
               [(0, [(gpus(2), [0])]), (1, [(gpus(1), [0])]), (2, [(gpus(4), [0])])],
               [(0, 9, [(1, gpus(4, 1000, GiB), 0)])],
               [(0, 0, [0, 1, 2])])
    return pc, ([3], [0b100], [1], [0])


def trap_outside():
    """Victim 0 holds 4 GPUs on node 0 (rack 0) and 4 on node 1 (rack 1); nothing is free.  In either rack its release
    frees only the 4 GPUs there: a job of 4 GPUs fits after it, a job of 8 never."""
    pc = _trap([[64000, 64000], [64 * GiB, 64 * GiB], [0, 0], [0, 0]], [0, 1], 2,
               [(0, [(gpus(4), [0, 1])])],
               [(0, 9, [(1, gpus(4, 1000, GiB), 0)]), (0, 9, [(1, gpus(8, 1000, GiB), 0)])],
               [(0, 0, [0]), (0, 1, [0]), (1, 0, [0]), (1, 1, [0])])
    return pc, ([1, 1, -1, -1], [1, 1, 0, 0], [1, 1, -1, -1], [0, -1])


def trap_best():
    """Three racks of one node, nothing free.  Rack 0 holds two victims of 2 GPUs, racks 1 and 2 one victim of 4 each.
    Job 0 (4 GPUs) needs two evictions in its first pair and one in its second: the second.  Job 1 has one eviction
    in both of its pairs: the smaller p."""
    pc = _trap([[64000] * 3, [64 * GiB] * 3, [0] * 3, [0] * 3], [0, 1, 2], 3,
               [(0, [(gpus(2), [0])]), (1, [(gpus(2), [0])]), (2, [(gpus(4), [1])]), (3, [(gpus(4), [2])])],
               [(0, 9, [(1, gpus(4, 1000, GiB), 0)]), (0, 9, [(1, gpus(4, 1000, GiB), 0)])],
               [(0, 0, [0, 1]), (0, 1, [2]), (1, 2, [3]), (1, 1, [2])])
    return pc, ([2, 1, 1, 1], [0b11, 1, 1, 1], [2, 1, 1, 1], [1, 2])


def trap_hopeless():
    """A needed label that no node has: whoever goes, the job is not placed.  prefix -1, count -1, mask 0."""
    pc = _trap([[64000], [64 * GiB], [0], [0]], [0], 1,
               [(0, [(gpus(8), [0])])],
               [(0, 9, [(1, gpus(1, 1000, GiB), DP.NO_LABEL)])],
               [(0, 0, [0])])
    return pc, ([-1], [0], [-1], [-1])


TRAPS = {"non_monotone": trap_non_monotone, "fill_back": trap_fill_back, "outside": trap_outside, "best": trap_best,
         "hopeless": trap_hopeless}


def check_engine(eng, pc, load=True, python=False, want=None):
    """Load the case (unless the engine already holds it), run the call and compare every prefix, victims, count and
    best cell with the checker (the oracle statement; the Python statement too where asked), and the residuals before
    and after.  Returns the checker's answer."""
    c = pc.case
    if load:
        eng.load_nodes(c.cap, c.used, c.labels, c.island)
    before = eng.read_residuals()
    if want is None:
        want = pc.answers(before)
    got = eng.gang_preempt_domains(*pc.call_args())
    for name, g, w in zip(("prefix", "victims", "count", "best"), got, want):
        assert np.array_equal(g, w), (name, np.nonzero(np.asarray(g) != np.asarray(w))[0][:10].tolist())
    if python:
        for g, w in zip(got, pc.answers(before, judge_python)):
            assert np.array_equal(g, w)
    assert np.array_equal(eng.read_residuals(), before)
    return want
