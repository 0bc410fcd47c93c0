"""Checker for pe_drain_fit_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): candidate c drains node n = cand_node[c] into the level-`level` domain D =
cand_domain[c].  Its evicted pods are the pod slots s of the book with pod_node[s] == n, ascending; consecutive evicted
slots of one group are a run (a group of count r); the answer is pe_place_greedy_domains' for the single job whose
groups are the runs, in D, on an inventory in which n is a removed slot.  Two statements of it:

    drain_oracle(...)   per candidate, gang_fit.answer_oracle (fits, the failing run, the pods placed) and the C
                        oracle's pod nodes on the domain's nodes without n, the runs as one job
    drain_python(...)   pod by pod in Python integers with semantics.appendix_b_key; `variant` switches in one of
                        the WRONG readings of the rule (VARIANTS), each of which must change some cell

Both return (fits uint8[C], moved int64[C], fail_slot int64[C], target int32[S]).

`labels` are the engine's labels: synth.island_labels applied.  A removed slot has NEVER in all four residuals.
"""
from dataclasses import dataclass

import numpy as np

import domain_placement as DP
import gang_fit as GF
import oracle
from oracle import semantics as S

ISLAND = DP.ISLAND
NEVER = -(1 << 63)
GiB = 1 << 30

# the wrong readings drain_python can be switched to
VARIANTS = ("node_kept",          # n not excluded
            "given_back",         # n's pods first given back to n, which then stays in the decisions: release, then place
            "descending",         # slots in descending order
            "island_split",       # an island run split into pods
            "island_group_count",   # an island run sized by group_count where fewer of its pods sit on n
            "other_nodes",        # the slots of the run's group on other nodes included
            "own_domain",         # cand_domain replaced by n's own domain
            "all_excluded",       # every candidate of the call excluded at once
            "need_ignored",       # need ignored
            "level0",             # level 0 whatever `level` says
            "targets_kept")       # targets of a failing candidate kept


@dataclass
class Book:
    """Placed gangs in pe_release_gangs' shape, plus the groups' need."""
    off: np.ndarray      # int32 [V + 1]
    cnt: np.ndarray      # int32 [VG]
    req: np.ndarray      # int64 [VG][4]
    need: np.ndarray     # uint32 [VG]
    pod: np.ndarray      # int32 [S]

    def args(self):
        return self.off, self.cnt, self.req, self.need, self.pod

    def group_of_slot(self):
        return np.repeat(np.arange(len(self.cnt)), np.clip(self.cnt, 0, None))


def make_book(gangs):
    """Book of [[(request[4], need, [node per pod slot]), ...], ...]: one list of groups per gang."""
    off, cnt, req, need, pod = [0], [], [], [], []
    for groups in gangs:
        for q, nd, nodes in groups:
            cnt.append(len(nodes))
            req.append(q)
            need.append(nd)
            pod += [int(x) for x in nodes]
        off.append(len(cnt))
    return Book(np.array(off, dtype=np.int32), np.array(cnt, dtype=np.int32), np.array(req, dtype=np.int64).reshape(-1, 4),
                np.array(need, dtype=np.uint32), np.array(pod, dtype=np.int32))


def runs_of(book, slots, group_of):
    """[(group, [slots])]: consecutive entries of `slots` that belong to one group."""
    out = []
    for s in slots:
        g = int(group_of[s])
        if out and out[-1][0] == g:
            out[-1][1].append(int(s))
        else:
            out.append((g, [int(s)]))
    return out


def removed(res, n):
    return int(res[0][n]) == NEVER


# ---------------------------------------------------------------- the oracle statement

def _oracle_pods(res, labels, nodes, groups):
    """The C oracle's pod nodes (global ids) of the one job `groups` on the sub-inventory `nodes`; it is placed."""
    cnt = np.array([c for c, _, _ in groups], dtype=np.int32)
    req = np.array([q for _, q, _ in groups], dtype=np.int64).reshape(-1, 4)
    need = np.array([nd for _, _, nd in groups], dtype=np.uint32)
    pods, st, _ = oracle.place_greedy(np.asarray(res)[:, nodes], np.asarray(labels)[nodes], np.array([0, len(groups)], dtype=np.int32),
                                      np.zeros(1, dtype=np.int32), cnt, req, need)
    assert int(st[0]) == 0
    return np.asarray(nodes)[pods]


def drain_oracle(res, labels, island, book, cand_node, cand_domain, level, level_size, parent):
    res = np.asarray(res, dtype=np.int64)
    members = GF.members_of(island, level, level_size, parent)
    group_of = book.group_of_slot()
    C, Sn = len(cand_node), len(book.pod)
    fits, moved = np.ones(C, dtype=np.uint8), np.zeros(C, dtype=np.int64)
    fail, target = np.full(C, -1, dtype=np.int64), np.full(Sn, -1, dtype=np.int32)
    none = np.zeros(0, dtype=np.int64)
    for c, (n, d) in enumerate(zip(cand_node, cand_domain)):
        n, d = int(n), int(d)
        if removed(res, n):
            continue
        runs = runs_of(book, np.nonzero(book.pod == n)[0], group_of)
        if not runs:
            continue
        nodes = members.get(d, none)
        nodes = nodes[nodes != n]
        groups = [(len(sl), [int(x) for x in book.req[g]], int(book.need[g])) for g, sl in runs]
        f, fg, pods = GF.answer_oracle(res, labels, nodes, groups)
        fits[c], moved[c] = f, pods
        if f:
            target[np.concatenate([sl for _, sl in runs])] = _oracle_pods(res, labels, nodes, groups)
        else:
            before = sum(len(sl) for _, sl in runs[:fg])
            fail[c] = runs[fg][1][pods - before]
    return fits, moved, fail, target


# ---------------------------------------------------------------- the Python statement

def drain_python(res, labels, island, book, cand_node, cand_domain, level, level_size, parent, variant=None):
    assert variant is None or variant in VARIANTS
    lvl = 0 if variant == "level0" else level
    dom = DP.dom_level(island, lvl, level_size, parent)
    members = {}
    for i, d in enumerate(dom):
        members.setdefault(int(d), []).append(i)
    group_of = book.group_of_slot()
    first_slot = np.concatenate([[0], np.cumsum(np.clip(book.cnt, 0, None))])
    C, Sn = len(cand_node), len(book.pod)
    fits, moved = np.ones(C, dtype=np.uint8), np.zeros(C, dtype=np.int64)
    fail, target = np.full(C, -1, dtype=np.int64), np.full(Sn, -1, dtype=np.int32)
    everyone = set(int(x) for x in cand_node)
    for c, (n, d) in enumerate(zip(cand_node, cand_domain)):
        n, d = int(n), int(d)
        if removed(res, n):
            continue
        if variant == "own_domain":
            d = int(dom[n])
        slots = [int(s) for s in np.nonzero(book.pod == n)[0]]
        if variant == "other_nodes":
            groups_here = sorted(set(int(group_of[s]) for s in slots))
            slots = [s for g in groups_here for s in range(int(first_slot[g]), int(first_slot[g + 1])) if book.pod[s] >= 0]
        if variant == "descending":
            slots = slots[::-1]
        out = {n} if variant not in ("node_kept", "given_back") else set()
        if variant == "all_excluded":
            out = everyone
        R = {i: [int(res[k][i]) for k in range(4)] for i in members.get(d, []) if i not in out}
        if variant == "given_back" and n in R:
            for s in slots:
                R[n] = [r + int(q) for r, q in zip(R[n], book.req[group_of[s]])]

        def argmin(q, need):
            best = None
            for i, r in R.items():
                k = S.appendix_b_key(r, int(labels[i]), q, need, i)
                if k is not None and (best is None or k < best):
                    best = k
            return best

        done = []                                           # (slot, node) in placement order
        for g, sl in runs_of(book, slots, group_of):
            q, need = [int(x) for x in book.req[g]], int(book.need[g])
            if variant == "need_ignored":
                need &= ISLAND
            unit = bool(need & ISLAND) and variant != "island_split"
            if unit:
                r = int(book.cnt[g]) if variant == "island_group_count" else len(sl)
                qe = [x * r for x in q]
                best = argmin(qe, need) if all(v <= S.INT64_MAX for v in qe) else None
                if best is None:
                    fits[c], fail[c] = 0, sl[0]
                    break
                i = best & 0xFFFFFF
                R[i] = [a - b for a, b in zip(R[i], qe)]
                done += [(s, i) for s in sl]
                continue
            for s in sl:
                best = argmin(q, need)
                if best is None:
                    fits[c], fail[c] = 0, s
                    break
                i = best & 0xFFFFFF
                R[i] = [a - b for a, b in zip(R[i], q)]
                done.append((s, i))
            if not fits[c]:
                break
        moved[c] = len(done)
        if fits[c] or variant == "targets_kept":
            for s, i in done:
                target[s] = i
    return fits, moved, fail, target


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def residual_after_move(res, book, target, node):
    """The residuals after the move of `node` was carried out: its pods' requests back to it, and off their targets."""
    res = np.array(res, dtype=np.int64, copy=True)
    group_of = book.group_of_slot()
    for s in np.nonzero(book.pod == node)[0]:
        res[:, node] += book.req[group_of[s]]
        res[:, int(target[s])] -= book.req[group_of[s]]
    return res


# ---------------------------------------------------------------- shared inputs

@dataclass
class DrainCase:
    case: DP.Case           # inventory and hierarchy; case.level is the call's level
    res: np.ndarray         # int64 [4][N]: the residuals the call sees (the book's gangs placed, `gone` removed)
    book: Book
    cand_node: np.ndarray
    cand_domain: np.ndarray
    gone: list              # nodes removed after the book was made (PE_NODE_REMOVE)

    def call_args(self):
        c = self.case
        return (*self.book.args(), self.cand_node, self.cand_domain, c.level, c.level_size, c.parent)

    def checker_args(self):
        c = self.case
        return (self.res, c.labels, c.island, self.book, self.cand_node, self.cand_domain, c.level, c.level_size, c.parent)


FILL = [8000, 0, 0, 0]
TINY = [1, 0, 0, 0]


def fillers(case, res, max_domains=6, slack=2):
    """Per domain (the first max_domains with room for more than `slack` pods of FILL) one job of all the FILL pods its
    nodes hold but `slack`: a node that holds more of them than that cannot be drained into its own domain."""
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    usable = (np.asarray(res) >= 0).all(axis=0)
    jobs = []
    for d in range(int(case.level_size[case.level])):
        room = int((res[0][usable & (dom == d)] // FILL[0]).sum())
        if room > slack and len(jobs) < max_domains:
            jobs.append((d, 0, [(room - slack, FILL, 0)]))
    return jobs


def resident_book(case, rounds=3):
    """Really place the case's job mix and `rounds` further mixes on the CPU (domain_placement.place): the placed jobs
    that hold a pod are the book, groups, needs and pod slots exactly as the placement returned them, so that nodes
    hold pods of several gangs interleaved.  Returns (Book, the residuals that remain)."""
    res = case.residual()
    gangs, first = [], []
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    populated = np.unique(dom[dom >= 0])
    batch, job_domain = case.batch, case.job_domain
    for r in range(rounds + 3):
        if r == rounds + 1:                                 # then the fillers: half the domains (one at least, six at
            batch, job_domain = DP.make_batch(fillers(case, res, min(6, max(1, len(populated) // 2))))   # most) are left
        if r == rounds + 2:                                 # with room for two pods of FILL: a drain there moves two
            # last, one pod of TINY per domain: it sits on its domain's best fit, and that node stays the best fit.
            # These gangs come FIRST in the book, so that the pod is the first its node evicts
            batch, job_domain = DP.make_batch([(int(d), 0, [(1, TINY, 0)]) for d in populated[:6]])
        pods, status, res = DP.place(res, case.labels, case.island, batch, job_domain, case.level, case.level_size, case.parent)
        poff = DP.pod_offsets(batch.group_count)
        for j in np.nonzero(status == 0)[0]:
            g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
            if poff[g1] > poff[g0]:
                (first if r == rounds + 2 else gangs).append(
                    [([int(x) for x in batch.group_req[g]], int(batch.group_need[g]), pods[poff[g]:poff[g + 1]].tolist())
                     for g in range(g0, g1)])
        batch, job_domain = DP.job_mix(res, case.labels, case.island, case.level, case.level_size, case.parent, 577 + 17 * r)
    return make_book(first + gangs), res


def candidates(case, book, res, seed, max_cands=24):
    """(cand_node, cand_domain, gone): up to max_cands nodes that hold a pod, most into their own domain, every third
    into another populated domain and one into an empty domain (where the level has one); two nodes without pods;
    and two nodes that are removed after the book was made, one of them holding pods."""
    rng = np.random.default_rng(seed)
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    n_dom = int(case.level_size[case.level])
    size = np.bincount(dom[dom >= 0], minlength=n_dom)
    populated, empty = np.nonzero(size > 0)[0], np.nonzero(size == 0)[0]
    holders = np.unique(book.pod[book.pod >= 0])
    picked = [int(x) for x in rng.permutation(holders)[:max_cands]]
    # the nodes that hold pods of two gangs, and island runs, first: every case shows them
    gang_of = np.repeat(np.arange(len(book.off) - 1), np.diff(book.off))[book.group_of_slot()]
    multi = [int(n) for n in holders if len(set(gang_of[book.pod == n])) >= 2][:4]
    isl = [int(n) for n in np.unique(book.pod[(book.need[book.group_of_slot()] & ISLAND) != 0])][:4]
    fill = (book.req[book.group_of_slot()] == np.array(FILL)).all(axis=1) & (book.pod >= 0)
    heavy = [int(n) for n in np.nonzero(np.bincount(book.pod[fill], minlength=len(dom)) >= 3)[0]][:4]   # more than the slack
    # ... and nodes that are themselves the best fit of their first pod in their own domain: the exclusion shows
    tiny = (book.req[book.group_of_slot()] == np.array(TINY)).all(axis=1) & (book.pod >= 0)
    best = [int(n) for n in np.unique(book.pod[tiny])][:2]
    picked = list(dict.fromkeys(heavy[:1] + best[:1] + heavy[1:] + best[1:] + multi + isl + picked))[:max_cands]
    node, domain = [], []
    for k, n in enumerate(picked):
        own = int(dom[n]) if dom[n] >= 0 else int(populated[0])
        d = own
        if k % 3 == 2 and len(populated) > 1:
            d = int(rng.choice(populated[populated != own]))
        node.append(n)
        domain.append(d)
    if len(empty) and picked:
        node.append(int(rng.choice([x for x in holders if x not in node] or [-1])))
        domain.append(int(empty[0]))
        if node[-1] < 0:
            node.pop(), domain.pop()
    free = [int(x) for x in np.setdiff1d(np.arange(len(dom)), holders)]
    for n in free[:2]:
        node.append(n)
        domain.append(int(dom[n]) if dom[n] >= 0 else int(populated[0]))
    gone = []
    if len(picked) >= 2:
        gone.append(picked[-1])                             # a candidate on a removed slot, with pods
    if len(free) > 2:
        gone.append(free[2])                                # a removed node that is no candidate: a hole in a domain
    return np.array(node, dtype=np.int32), np.array(domain, dtype=np.int32), gone


def tree_drain_case(name, n, level, seed=67):
    """A named hierarchy with a resident book, candidates and removed slots (the shared input of both tests)."""
    case = DP.tree_case(name, n, level)
    book, res = resident_book(case)
    node, domain, gone = candidates(case, book, res, seed + 5 * level + n)
    res = np.array(res, copy=True)
    for g in gone:
        res[:, g] = NEVER
    return DrainCase(case, res, book, node, domain, gone)


def load_engine(eng, dc):
    """The engine holds the residuals the case's call sees: loaded with `used` such that cap - used is dc.res, the
    removed slots loaded live and then removed (PE_NODE_REMOVE)."""
    c = dc.case
    res = np.array(dc.res, copy=True)
    res[:, dc.gone] = c.residual()[:, dc.gone]
    eng.load_nodes(c.cap, c.cap - res, c.labels, c.island)
    if dc.gone:
        eng.update_nodes(dc.gone, [1] * len(dc.gone))
    assert np.array_equal(eng.read_residuals(), dc.res)


def check_engine(eng, dc, load=True, python=False):
    """Load the case (unless the engine already holds it), run the call and compare every cell of all four outputs
    with the checker (the oracle statement, and the Python statement too where asked).  The residuals must come out
    as they went in.  Returns the checker's (fits, moved, fail_slot, target)."""
    if load:
        load_engine(eng, dc)
    want = drain_oracle(*dc.checker_args())
    got = eng.drain_fit_domains(*dc.call_args())
    for a, b, what in zip(got, want, ("fits", "moved", "fail_slot", "target")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, np.nonzero(a != b)[0][:10].tolist())
    if python:
        assert same(got, drain_python(*dc.checker_args()))
    assert np.array_equal(eng.read_residuals(), dc.res)
    return want


def flat_case(free_gpus, island=None, labels=None, cpu=64000, mem=256 * GiB):
    """A Case of len(free_gpus) nodes with that many free GPUs each, cpu and memory equal and ample, nothing used;
    island: the nodes' leaf domains (default: one rack)."""
    n = len(free_gpus)
    cap = np.array([[cpu] * n, [mem] * n, list(free_gpus), [0] * n], dtype=np.int64)
    isl = np.zeros(n, dtype=np.int32) if island is None else np.array(island, dtype=np.int32)
    lab = np.full(n, 1 | ISLAND, dtype=np.uint32) if labels is None else np.array(labels, dtype=np.uint32)
    batch, job_domain = DP.make_batch([])
    return DP.Case(cap, np.zeros_like(cap), lab, isl, [int(isl.max()) + 1], None, 0, batch, job_domain)


def gpus(g, cpu=1000):
    return [cpu, GiB, g, 0]


def traps():
    """{name: (DrainCase, expected or None)}: hand-made inputs; expected = (fits, moved, fail_slot, target) lists."""
    out = {}

    def add(name, case, gangs, node, domain, expected=None, gone=()):
        res = case.residual()
        for g in gone:
            res[:, g] = NEVER
        out[name] = (DrainCase(case, res, make_book(gangs), np.array(node, dtype=np.int32), np.array(domain, dtype=np.int32),
                               list(gone)), expected)

    A, B, Cn = 0, 1, 2
    rack = flat_case([0, 3, 4])
    # the worked example, both ways
    add("worked_fails", rack, [[(gpus(2), 0, [A, A])], [(gpus(3), 0, [A])]], [A], [0], ([0], [2], [2], [-1, -1, -1]))
    add("worked_fits", rack, [[(gpus(3), 0, [A])], [(gpus(2), 0, [A, A])]], [A], [0], ([1], [3], [-1], [B, Cn, Cn]))
    # the excluded node would have been the argmin: A has 2 free GPUs, the tightest fit for its own 2-GPU pod
    add("argmin_excluded", flat_case([2, 5, 6]), [[(gpus(2), 0, [A])]], [A], [0], ([1], [1], [-1], [B]))
    # two candidates in one unit, the second's pod has the first's node as its argmin: a stale exclusion shows
    add("stale_exclusion", flat_case([2, 3, 8]), [[(gpus(2), 0, [A])], [(gpus(2), 0, [B])]], [A, B], [0, 0],
        ([1, 1], [1, 1], [-1, -1], [B, A]))
    # a candidate that fills the domain and fails, followed by one that needs the same slots: a stale copy shows
    add("stale_copy", flat_case([0, 0, 4]), [[(gpus(2), 0, [A, A, A])], [(gpus(4), 0, [B])]], [A, B], [0, 0],
        ([0, 1], [2, 1], [2, -1], [-1, -1, -1, Cn]))
    # the target domain is another rack; and the node's own rack has no other node
    two = flat_case([0, 4, 4], island=[0, 1, 1])
    add("other_rack", two, [[(gpus(2), 0, [A])]], [A], [1], ([1], [1], [-1], [B]))
    add("alone_in_rack", two, [[(gpus(2), 0, [A])]], [A], [0], ([0], [0], [0], [-1]))
    add("alone_no_pods", two, [[(gpus(2), 0, [B])]], [A], [0], ([1], [0], [-1], [-1]))
    # island runs: one that fits a node whole, one that fits none although the pods alone would, one whose product
    # overflows; and a group of three whose pods sit on two nodes: the run is the 2 pods on A, not the group's 3
    add("island_fits", flat_case([0, 3, 4]), [[(gpus(2), ISLAND, [A, A])]], [A], [0], ([1], [2], [-1], [Cn, Cn]))
    add("island_fits_none", flat_case([0, 3, 3]), [[(gpus(2), ISLAND, [A, A])]], [A], [0], ([0], [0], [0], [-1, -1]))
    add("island_overflow", flat_case([0, 3, 4]), [[(gpus(1), 0, [A]), ([1 << 62, 0, 0, 0], ISLAND, [A, A])]], [A], [0],
        ([0], [1], [1], [-1, -1, -1]))
    add("island_part", flat_case([0, 4, 5]), [[(gpus(2), ISLAND, [A, B, A])]], [A], [0], ([1], [2], [-1], [B, -1, B]))
    # labels: the pod needs bit 1, only C has it
    add("need", flat_case([0, 3, 8], labels=[1 | ISLAND, 1 | ISLAND, 3 | ISLAND]), [[(gpus(2), 2, [A])]], [A], [0],
        ([1], [1], [-1], [Cn]))
    # zero-request pods fit every live node but not a removed one; skipped slots; a candidate on a removed slot
    add("zero_request", flat_case([0, 0, 0]), [[([0, 0, 0, 0], 0, [A, -1, A])]], [A], [0], ([1], [2], [-1], [B, -1, B]))
    add("zero_request_removed", flat_case([0, 0, 0]), [[([0, 0, 0, 0], 0, [A])]], [A], [0], ([0], [0], [0], [-1]), gone=(B, Cn))
    add("candidate_removed", flat_case([0, 3, 4]), [[(gpus(2), 0, [A, A])]], [A, B], [0, 0], ([1, 1], [0, 0], [-1, -1], [-1, -1]),
        gone=(A,))
    # pods of two gangs interleaved with another node's: runs are consecutive in the EVICTED list, by group
    add("interleaved", flat_case([0, 4, 4, 9]), [[(gpus(2), 0, [A, B, A])], [(gpus(1), 0, [B, A])]], [A, B], [0, 0])
    return out
