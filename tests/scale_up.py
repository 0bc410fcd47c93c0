"""Checker for pe_scale_up_domains and the inputs its CPU and GPU tests share.

The rule (include/placement.h): attempt k of pair p is pe_gang_fit_domains' judgement of job pair_job[p] in domain
pair_domain[p] on the domain's nodes with their current residuals plus k new members -- new node i < k with the
residual of template pair_template[p], its labels with bit 31 set and id new_slot[i].  The attempts run in ascending
k and the first that places the job is the answer; the deciding attempt (that one, or attempt pair_max[p]) gives
fail_group, pods and new_pods.  Two statements of it:

    scale_oracle(...)   per attempt gang_fit.answer_oracle (the C oracle) on the sub-inventory of the domain's members
                        and the k new nodes, in ascending id; new_pods from the oracle's pods of the job cut to what
                        the attempt placed
    scale_python(...)   pod by pod in Python integers with semantics.appendix_b_key (small inputs); with `variant` it
                        states one of the wrong readings in VARIANTS, each a fault the kernel or the host could have

`labels` are the engine's labels: synth.island_labels applied.  A removed slot has NEVER in all four residuals and is
in no domain, whatever the case's island array says about it.
"""
from dataclasses import dataclass

import numpy as np

import domain_placement as DP
import gang_fit as GF
import oracle
from oracle import semantics as S
from placement import synth

ISLAND = DP.ISLAND
NEVER = -(1 << 63)
GiB = DP.GiB
ONLY_NEW = DP.NO_LABEL      # a label bit no inventory here sets: a group that needs it is held by template nodes only

VARIANTS = ("descending", "bisect", "new_lose", "new_win", "no_island_bit", "labels_ignored", "stale_new", "stale_real",
            "n_new_for_max", "template0", "k_off_by_one", "new_pods_takes", "attempt0_outputs", "best_smallest_p",
            "empty_domain_no")


@dataclass
class ScaleCase:
    case: DP.Case             # the inventory's shape, the hierarchy, the level and the batch
    res: np.ndarray           # int64 [4][N]: the residuals the call sees, removed slots NEVER
    gone: list                # the removed slots (PE_NODE_REMOVE after the load)
    tmpl_res: np.ndarray      # int64 [T][4]
    tmpl_labels: object       # uint32 [T] or None
    new_slot: np.ndarray      # int32 [n_new]
    pair_job: np.ndarray
    pair_domain: np.ndarray
    pair_template: np.ndarray
    pair_max: object          # int32 [P] or None = n_new

    def kmax(self):
        n_new = len(self.new_slot)
        return np.full(len(self.pair_job), n_new, dtype=np.int32) if self.pair_max is None else self.pair_max

    def call_args(self):
        b, c = self.case.batch, self.case
        return (b.job_group_off, b.group_count, b.group_req, b.group_need, self.tmpl_res, self.tmpl_labels, self.new_slot,
                self.pair_job, self.pair_domain, self.pair_template, self.pair_max, c.level, c.level_size, c.parent)


def live_members(sc):
    """{domain: ascending ids of its nodes that are not removed slots}."""
    c = sc.case
    members = GF.members_of(c.island, c.level, c.level_size, c.parent)
    return {d: n[sc.res[0][n] != NEVER] for d, n in members.items()}


def best_of(pair_job, nodes, J):
    """int32[J]: the pair of job j with the smallest nodes >= 0, ties to the smallest p, -1 when there is none."""
    best = np.full(J, -1, dtype=np.int32)
    for p in range(len(pair_job) - 1, -1, -1):
        j = int(pair_job[p])
        if nodes[p] >= 0 and (best[j] < 0 or nodes[p] <= nodes[best[j]]):
            best[j] = p
    return best


def _tmpl_label(sc, t):
    return (0 if sc.tmpl_labels is None else int(sc.tmpl_labels[t])) | ISLAND


# ---------------------------------------------------------------- the oracle statement

def attempt_oracle(sc, nodes, groups, t, k):
    """(fits, fail_group, pods, new_pods) of attempt k: the C oracle on the members and k new nodes in ascending id."""
    ids = np.concatenate([np.asarray(nodes, dtype=np.int64), sc.new_slot[:k].astype(np.int64)])
    order = np.argsort(ids, kind="stable")
    R = np.concatenate([sc.res[:, nodes], np.repeat(np.asarray(sc.tmpl_res[t], dtype=np.int64)[:, None], k, axis=1)], axis=1)[:, order]
    L = np.concatenate([np.asarray(sc.case.labels, dtype=np.uint32)[nodes], np.full(k, _tmpl_label(sc, t), dtype=np.uint32)])[order]
    is_new = (np.arange(len(ids)) >= len(nodes))[order]
    f, fg, pods = GF.answer_oracle(R, L, np.arange(len(ids)), groups)
    cut = list(groups)
    if not f:                                               # the job cut to what the attempt placed is placed
        before = sum(max(c, 0) for c, _, _ in groups[:fg])
        cut = list(groups[:fg]) + ([(pods - before, groups[fg][1], groups[fg][2])] if pods > before else [])
    new_pods = 0
    if pods > 0:
        cnt = np.array([c for c, _, _ in cut], dtype=np.int32)
        req = np.array([q for _, q, _ in cut], dtype=np.int64).reshape(-1, 4)
        need = np.array([nd for _, _, nd in cut], dtype=np.uint32)
        pn, st, _ = oracle.place_greedy(R, L, np.array([0, len(cut)], dtype=np.int32), np.zeros(1, dtype=np.int32), cnt, req, need)
        assert int(st[0]) == 0 and len(pn) == pods
        new_pods = int(is_new[pn].sum())
    return f, fg, pods, new_pods


def scale_oracle(sc):
    """(nodes int32[P], fail_group int32[P], pods int64[P], new_pods int64[P], best int32[J])."""
    members = live_members(sc)
    none = np.zeros(0, dtype=np.int64)
    b = sc.case.batch
    P, J = len(sc.pair_job), len(b.job_group_off) - 1
    nodes, fail = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
    pods, newp = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    memo = {}
    for p, (j, d, t, K) in enumerate(zip(sc.pair_job, sc.pair_domain, sc.pair_template, sc.kmax())):
        key = (int(j), int(d), int(t), int(K))
        if key not in memo:
            groups = GF.job_groups(b, int(j))
            ans = None
            for k in range(int(K) + 1):
                f, fg, pd, nw = attempt_oracle(sc, members.get(int(d), none), groups, int(t), k)
                ans = (k if f else -1, fg, pd, nw)
                if f:
                    break
            memo[key] = ans
        nodes[p], fail[p], pods[p], newp[p] = memo[key]
    return nodes, fail, pods, newp, best_of(sc.pair_job, nodes, J)


# ---------------------------------------------------------------- the Python statement

def _walk(places, groups):
    """The groups' walk over places {key id: (residual list, labels, is_new)}, residuals mutated: (fits, fail_group,
    pods, pods on new places, takes on new places); a take is one decision."""
    def argmin(q, need):
        best = None
        for kid, (r, lab, _) in places.items():
            k = S.appendix_b_key(r, lab, q, need, kid)
            if k is not None and (best is None or k < best):
                best = k
        return best

    pods = new_pods = new_takes = 0
    for g, (c, q, need) in enumerate(groups):
        if c <= 0:
            continue
        if need & ISLAND:
            qe = [x * c for x in q]
            best = argmin(qe, need) if all(v <= S.INT64_MAX for v in qe) else None
            if best is None:
                return 0, g, pods, new_pods, new_takes
            r, _, new = places[best & 0xFFFFFF]
            r[:] = [a - v for a, v in zip(r, qe)]
            pods += c
            new_pods += c * new
            new_takes += new
            continue
        last = None
        for _ in range(c):
            best = argmin(q, need)
            if best is None:
                return 0, g, pods, new_pods, new_takes
            kid = best & 0xFFFFFF
            r, _, new = places[kid]
            r[:] = [a - v for a, v in zip(r, q)]
            pods += 1
            new_pods += new
            new_takes += new and kid != last                # consecutive pods on one node are one take
            last = kid
    return 1, -1, pods, new_pods, new_takes


def attempt_python(sc, nodes, groups, t, k):
    """(fits, fail_group, pods, new_pods) of attempt k alone."""
    places = {int(n): ([int(sc.res[d][n]) for d in range(4)], int(sc.case.labels[n]), 0) for n in nodes}
    for i in range(k):
        places[int(sc.new_slot[i])] = ([int(x) for x in sc.tmpl_res[t]], _tmpl_label(sc, t), 1)
    return _walk(places, groups)[:4]


def pair_python(sc, nodes, groups, t, K, variant=None):
    """(nodes, fail_group, pods, new_pods) of one pair."""
    n_new = len(sc.new_slot)
    if variant == "n_new_for_max":
        K = n_new
    if variant == "template0":
        t = 0
    tres = [int(x) for x in sc.tmpl_res[t]]
    tlab = _tmpl_label(sc, t)
    if variant == "no_island_bit":
        tlab &= ~ISLAND
    if variant == "labels_ignored":
        tlab = ISLAND
    real_kid = (lambda n: n + 64) if variant == "new_win" else (lambda n: n)
    new_kid = ((lambda i: 0xFFFFC0 + i) if variant == "new_lose" else (lambda i: i) if variant == "new_win"
               else (lambda i: int(sc.new_slot[i])))
    state = {"real": None, "new": {}}
    done = {}

    def run(k):
        if k in done:
            return done[k]
        if state["real"] is None or variant != "stale_real":
            state["real"] = {int(n): [int(sc.res[d][n]) for d in range(4)] for n in nodes}
        if variant != "stale_new":
            state["new"] = {}
        live = min(k + (variant == "k_off_by_one"), n_new)
        places = {real_kid(n): (r, int(sc.case.labels[n]), 0) for n, r in state["real"].items()}
        for i in range(live):
            places[new_kid(i)] = (state["new"].setdefault(i, list(tres)), tlab, 1)
        done[k] = _walk(places, groups)
        return done[k]

    if variant == "empty_domain_no" and len(nodes) == 0 and any(c > 0 for c, _, _ in groups):
        ans, decide = -1, 0
    elif variant == "descending":
        ans = -1
        if run(K)[0]:
            ans = K
            while ans > 0 and run(ans - 1)[0]:
                ans -= 1
        decide = ans if ans >= 0 else K
    elif variant == "bisect":
        if run(0)[0]:
            ans = 0
        elif not run(K)[0]:
            ans = -1
        else:
            lo, ans = 0, K
            while ans - lo > 1:
                mid = (lo + ans) // 2
                lo, ans = (lo, mid) if run(mid)[0] else (mid, ans)
        decide = ans if ans >= 0 else K
    else:
        ans = next((k for k in range(K + 1) if run(k)[0]), -1)
        decide = ans if ans >= 0 else K
    _, fg, pods, new_pods, new_takes = run(0 if variant == "attempt0_outputs" else decide)
    return ans, fg, pods, new_takes if variant == "new_pods_takes" else new_pods


def scale_python(sc, variant=None):
    """scale_oracle(...) by the Python statement, or by one of its wrong readings."""
    assert variant is None or variant in VARIANTS
    members = live_members(sc)
    b = sc.case.batch
    P, J = len(sc.pair_job), len(b.job_group_off) - 1
    nodes, fail = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
    pods, newp = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    memo = {}
    for p, (j, d, t, K) in enumerate(zip(sc.pair_job, sc.pair_domain, sc.pair_template, sc.kmax())):
        key = (int(j), int(d), int(t), int(K))
        if key not in memo:
            memo[key] = pair_python(sc, members.get(int(d), []), GF.job_groups(b, int(j)), int(t), int(K), variant)
        nodes[p], fail[p], pods[p], newp[p] = memo[key]
    if variant == "best_smallest_p":
        best = GF.first_of(sc.pair_job, nodes >= 0, J)
    else:
        best = best_of(sc.pair_job, nodes, J)
    return nodes, fail, pods, newp, best


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


NAMES = ("nodes", "fail_group", "pods", "new_pods", "best")


# ---------------------------------------------------------------- shared inputs

def extend_batch(batch, jobs):
    """The batch with jobs [[(count, request[4], need), ...], ...] appended; returns (batch, the new jobs' indices)."""
    more, _ = DP.make_batch([(0, 0, groups) for groups in jobs])
    G = len(batch.group_count)
    J = len(batch.priority)
    out = synth.JobBatch(np.concatenate([batch.job_group_off, more.job_group_off[1:] + G]).astype(np.int32),
                         np.concatenate([batch.priority, more.priority]).astype(np.int32),
                         np.concatenate([batch.group_count, more.group_count]).astype(np.int32),
                         np.concatenate([np.asarray(batch.group_req).reshape(-1, 4), more.group_req]).astype(np.int64),
                         np.concatenate([batch.group_need, more.group_need]).astype(np.uint32),
                         np.concatenate([batch.kind, more.kind]).astype(np.int8))
    return out, list(range(J, J + len(jobs)))


def spare_slots(n, count, seed):
    """`count` ids of [0, n) to be removed slots: the two lowest, the two highest, the rest anywhere between -- so
    that new ids lie below, between and above the live ones -- in a shuffled hand-out order."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, n - 2, n - 1][:count]
    rest = rng.choice(np.arange(2, n - 2), size=max(0, count - len(fixed)), replace=False).tolist() if n > 4 + count else []
    return [int(x) for x in rng.permutation(fixed + rest)]


# the templates of the tree cases: around the requests of domain_placement.job_mix.  Template 0 carries ONLY_NEW
_TEMPLATES = [([16000, 64 * GiB, 1, 50 * GiB], 0xF | ONLY_NEW), ([8000, 16 * GiB, 1, 10 * GiB], 0x3),
              ([2000, 4 * GiB, 0, 0], 0xE), ([32000, 128 * GiB, 2, 100 * GiB], 0xF)]


def tree_scale_case(name, n, level, seed=71, max_pairs=48, n_new=5):
    """A named hierarchy with removed slots, templates and a pair mix (the shared input of both tests).  The pairs are
    gang_fit.pair_mix's, thinned to max_pairs, plus the pairs of three jobs made for the case: one that is placed as
    it is (answer 0), and one that only template-0 nodes hold, three of them -- asked with pair_max 2 first (answer
    -1) and then with 5 (answer 3, the job's best although not its first pair)."""
    case = DP.tree_case(name, n, level)
    rng = np.random.default_rng(seed + 13 * level + n)
    gone = spare_slots(n, n_new + 3, seed + n)
    res = np.array(case.residual(), copy=True)
    res[:, gone] = NEVER
    pj, pd = GF.pair_mix(case, seed + 11 * level + n)
    keep = np.sort(rng.permutation(len(pj))[:max_pairs])
    pj, pd = pj[keep], pd[keep]
    pt = rng.integers(0, len(_TEMPLATES), len(pj)).astype(np.int32)
    pm = rng.choice([0, 1, 2, n_new, n_new], len(pj)).astype(np.int32)
    t0 = _TEMPLATES[0][0]
    batch, (jz, jx) = extend_batch(case.batch, [[(1, [0, 0, 0, 0], 0)], [(3, t0, ONLY_NEW)]])
    sc0 = ScaleCase(case, res, gone, None, None, None, None, None, None, None)
    live = live_members(sc0)
    d0 = max(live, key=lambda d: (len(live[d]), -d))           # the domain with the most live nodes
    pj = np.concatenate([pj, [jz, jx, jx]]).astype(np.int32)
    pd = np.concatenate([pd, [d0, d0, d0]]).astype(np.int32)
    pt = np.concatenate([pt, [1, 0, 0]]).astype(np.int32)
    pm = np.concatenate([pm, [1, 2, n_new]]).astype(np.int32)
    case = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, case.parent, case.level, batch, case.job_domain)
    return ScaleCase(case, res, gone, np.array([t for t, _ in _TEMPLATES], dtype=np.int64),
                     np.array([lab for _, lab in _TEMPLATES], dtype=np.uint32), np.array(gone[:n_new], dtype=np.int32),
                     pj, pd, pt, pm)


def load_engine(eng, sc):
    """The engine holds the residuals the case's call sees: the removed slots loaded live and then removed."""
    c = sc.case
    eng.load_nodes(c.cap, c.used, c.labels, c.island)
    if sc.gone:
        eng.update_nodes(sc.gone, [1] * len(sc.gone))
    assert np.array_equal(eng.read_residuals(), sc.res)


def check_engine(eng, sc, load=True, python=False):
    """Load the case (unless the engine already holds it), run the call and compare every cell of all five outputs
    with the checker (the oracle statement, and the Python statement too where asked).  The residuals must come out
    as they went in.  Returns the checker's answer."""
    if load:
        load_engine(eng, sc)
    want = scale_oracle(sc)
    got = eng.scale_up_domains(*sc.call_args())
    for a, b, what in zip(got, want, NAMES):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, np.nonzero(a != b)[0][:10].tolist())
    if python:
        assert same(got, scale_python(sc))
    assert np.array_equal(eng.read_residuals(), sc.res)
    return want


def rack_case(free, spare, island=None, labels=None, n_dom=None):
    """A Case of len(free) live nodes with residual free[i] (4 cells, or (cpu m, GPUs) with memory and storage 0)
    followed by `spare` removed slots, nothing used; island: the live nodes' leaf domains (default: one rack); the
    removed slots' ids are len(free) .. len(free) + spare - 1 unless `free` holds None at other places: a None is a
    removed slot where it stands."""
    rows = [r if r is None or len(r) == 4 else [r[0], 0, r[1], 0] for r in free] + [None] * spare
    gone = [i for i, r in enumerate(rows) if r is None]
    cap = np.array([[0, 0, 0, 0] if r is None else r for r in rows], dtype=np.int64).T.copy()
    live = [i for i, r in enumerate(rows) if r is not None]
    isl = np.zeros(len(rows), dtype=np.int32)
    if island is not None:
        isl[live] = island
    lab = np.full(len(rows), 1 | ISLAND, dtype=np.uint32)
    if labels is not None:
        lab[live] = np.array(labels, dtype=np.uint32) | np.uint32(ISLAND)
    batch, job_domain = DP.make_batch([])
    case = DP.Case(cap, np.zeros_like(cap), lab, isl, [int(isl.max()) + 1 if n_dom is None else n_dom], None, 0, batch, job_domain)
    res = np.array(cap, copy=True)
    res[:, gone] = NEVER
    return case, res, gone


def make_case(free, spare, jobs, tmpl, new_slot, pairs, island=None, labels=None, n_dom=None, tmpl_labels=None):
    """jobs: [[(count, request, need), ...], ...] with requests of 4 cells or (cpu m, GPUs); tmpl: residuals alike;
    pairs: [(job, domain, template, max or None), ...] -- None for every pair gives pair_max None."""
    wide = lambda q: list(q) if len(q) == 4 else [q[0], 0, q[1], 0]   # noqa: E731
    case, res, gone = rack_case(free, spare, island, labels, n_dom)
    batch, _ = DP.make_batch([(0, 0, [(c, wide(q), nd) for c, q, nd in groups]) for groups in jobs])
    case = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, None, 0, batch, np.zeros(len(jobs), dtype=np.int32))
    pm = None if all(p[3] is None for p in pairs) else np.array([p[3] for p in pairs], dtype=np.int32)
    col = lambda k: np.array([p[k] for p in pairs], dtype=np.int32)   # noqa: E731
    return ScaleCase(case, res, gone, np.array([wide(t) for t in tmpl], dtype=np.int64).reshape(-1, 4),
                     None if tmpl_labels is None else np.array(tmpl_labels, dtype=np.uint32),
                     np.array(new_slot, dtype=np.int32), col(0), col(1), col(2), pm)


def gpus(g, cpu=1000):
    return [cpu, GiB, g, 0]


def node(g):
    """The free residual of a node or template with g GPUs, cpu and memory ample."""
    return [64000, 256 * GiB, g, 0]


# the non-monotone cases, each (free (cpu m, GPUs) per real node, template, groups (count, (cpu m, GPUs)), K, the k
# whose attempts place the job): the issue's, and others from a seeded search over random draws of 1-3 nodes and 2-4
# groups with this file's Python statement, run once; the new ids lie above the real ones
NON_MONOTONE = {
    "non_monotone_issue": ([(15000, 8), (14000, 7)], (9000, 2), [(2, (6000, 1)), (1, (7000, 7)), (1, (2000, 1)), (2, (8000, 0))],
                           4, [1, 3, 4]),
    "non_monotone_three_nodes": ([(13000, 5), (14000, 7), (8000, 3)], (7000, 5),
                                 [(2, (4000, 4)), (1, (6000, 4)), (2, (8000, 0)), (1, (8000, 3))], 4, [1, 3, 4]),
    "non_monotone_large_template": ([(14000, 7), (5000, 8)], (15000, 6),
                                    [(1, (7000, 4)), (1, (6000, 4)), (1, (2000, 5)), (1, (7000, 3))], 4, [1, 3, 4]),
    "non_monotone_from_zero": ([(6000, 3), (14000, 8), (16000, 6)], (7000, 3),
                               [(2, (4000, 1)), (1, (7000, 6)), (1, (7000, 2)), (2, (5000, 2))], 4, [0, 2, 3, 4]),
}


def traps():
    """{name: (ScaleCase, expected or None)}: hand-made inputs; expected = (nodes, fail_group, pods, new_pods, best)."""
    out = {}

    def add(name, expected, *args, **kw):
        out[name] = (make_case(*args, **kw), expected)

    # the header's worked example: one node with 8 free GPUs, a template of 4, A = 1 x 4 then B = 1 x 8
    add("worked", ([1], [-1], [2], [1], [0]), [node(8)], 2, [[(1, gpus(4), 0), (1, gpus(8), 0)]], [node(4)], [1, 2],
        [(0, 0, 0, None)])
    for name, (free, tmpl, groups, K, fit_ks) in NON_MONOTONE.items():
        add(name, ([fit_ks[0]], [-1], [sum(c for c, _ in groups)], None, [0]), free, K, [[(c, q, 0) for c, q in groups]],
            [tmpl], list(range(len(free), len(free) + K)), [(0, 0, 0, K)])
    # a real node whose residual equals the template's: a tie on score that the ids decide.  B needs bit 1, which only
    # the real node has.  New id 0 < real id 1: A goes to the new node and B to the real one.  New id 2 > real id 1:
    # A takes the real node, and B finds 5 GPUs there and no label on the new nodes, one or two of them
    tie = [[(1, gpus(3), 0), (1, gpus(8), 2)]]
    add("tie_new_below", ([1], [-1], [2], [1], [0]), [None, node(8), None], 1, tie, [node(8)], [0, 2], [(0, 0, 0, 2)],
        labels=[3], tmpl_labels=[1])
    add("tie_new_above", ([-1], [1], [1], [0], [-1]), [None, node(8), None], 1, tie, [node(8)], [2, 3], [(0, 0, 0, 2)],
        labels=[3], tmpl_labels=[1])
    # a template smaller than every real node: the new node is the tightest fit and is chosen first
    add("small_template", ([1], [-1], [3], [1], [0]), [node(16), node(16)], 2, [[(1, gpus(2), 0), (2, gpus(16), 0)]],
        [node(2)], [2, 3], [(0, 0, 0, 2)])
    # a group larger than the template: no number of nodes helps, and the failing group is that one
    add("larger_than_template", ([-1], [1], [1], [0], [-1]), [node(4)], 3, [[(1, gpus(4), 0), (1, gpus(8), 0)]], [node(4)],
        [1, 2, 3], [(0, 0, 0, 3)])
    # an island group that only a new node holds: 2 x 3 GPUs on one node, the real ones have 3 each
    add("island_on_new", ([1], [-1], [3], [2], [0]), [node(3), node(3)], 2, [[(1, gpus(3), 0), (2, gpus(3), ISLAND)]],
        [node(8)], [3, 2], [(0, 0, 0, 2)])
    # a need bit only the template has
    add("need_on_template", ([2], [-1], [2], [2], [0]), [node(8)], 2, [[(2, gpus(4), 4)]], [node(4)], [1, 2], [(0, 0, 0, 2)],
        tmpl_labels=[5])
    # the caller's bit 31 is replaced: a template without it still takes an island group
    add("island_bit_set", ([1], [-1], [2], [2], [0]), [node(1)], 1, [[(2, gpus(2), ISLAND)]], [node(4)], [1], [(0, 0, 0, 1)],
        tmpl_labels=[1])
    # a domain without nodes holds what k template nodes hold; a job without pods is placed there with none
    add("empty_domain", ([2, 0, -1], [-1, -1, 0], [2, 0, 1], [2, 0, 1], [0, 1]), [node(8)], 2,
        [[(2, gpus(4), 0)], [(0, gpus(4), 0)]], [node(4)], [1, 2], [(0, 1, 0, 2), (1, 1, 0, 2), (0, 1, 0, 1)], n_dom=2)
    # a product that overflows fits nowhere, new nodes or not
    add("island_overflow", ([-1], [1], [1], [0], [-1]), [node(8)], 2, [[(1, gpus(1), 0), (2, [1 << 62, 0, 0, 0], ISLAND)]],
        [[(1 << 63) - 1, GiB, 8, 0]], [1, 2], [(0, 0, 0, 2)])
    # two templates and unequal maxima for one job: the best pair is neither the first nor the first with an answer
    add("best_not_first", ([-1, 4, 2, -1], [0, -1, -1, 0], [1, 4, 4, 2], [1, 4, 4, 2], [2]), [node(0)], 4, [[(4, gpus(2), 0)]],
        [node(2), node(4)], [1, 2, 3, 4], [(0, 0, 0, 1), (0, 0, 0, 4), (0, 0, 1, 4), (0, 0, 1, 1)])
    return out


def sized_case(sizes, K, seed, pairs_per_domain=1, n_new=None):
    """One level whose domain d has sizes[d] nodes of the synth inventory, dealt in a shuffled order, with 70 more
    nodes in no domain of which the n_new (default max(K, 1)) new slots and a few others are removed: new ids below,
    between and above every segment's.  Per domain `pairs_per_domain` pairs of unequal pair_max <= K over three jobs:
    one that only template-0 nodes hold, K of them (answer K, or -1 below), one of mixed groups, and one that is
    placed as it is in a populated domain."""
    n_new = max(K, 1) if n_new is None else n_new
    case = DP.one_level_case(sizes, [], seed=seed, pad=70)
    rng = np.random.default_rng(seed)
    pad = np.nonzero(np.asarray(case.island) < 0)[0]
    gone = [int(x) for x in rng.permutation(pad)[:min(len(pad), n_new + 3)]]
    res = np.array(case.residual(), copy=True)
    res[:, gone] = NEVER
    t0 = _TEMPLATES[0][0]
    jobs = [[(max(K, 1), t0, ONLY_NEW)],
            [(2, [8000, 16 * GiB, 1, 0], 1), (3, [2000, 4 * GiB, 0, 0], 0), (1, t0, ONLY_NEW), (2, [16000, 64 * GiB, 1, 0], ISLAND)],
            [(1, [0, 0, 0, 0], 0)]]
    batch, _ = DP.make_batch([(0, 0, g) for g in jobs])
    case = DP.Case(case.cap, case.used, case.labels, case.island, case.level_size, None, 0, batch, np.zeros(3, dtype=np.int32))
    pj, pd, pt, pm = [], [], [], []
    for d in range(len(sizes)):
        for i in range(pairs_per_domain):
            pj.append(i % 3)
            pd.append(d)
            pt.append(0 if i % 3 == 0 else int(rng.integers(0, len(_TEMPLATES))))
            pm.append(K if i < 3 else int(rng.integers(0, K + 1)))
    order = rng.permutation(len(pj))
    col = lambda x: np.array(x, dtype=np.int32)[order]   # noqa: E731
    return ScaleCase(case, res, gone, np.array([t for t, _ in _TEMPLATES], dtype=np.int64),
                     np.array([lab for _, lab in _TEMPLATES], dtype=np.uint32), np.array(gone[:n_new], dtype=np.int32),
                     col(pj), col(pd), col(pt), col(pm))
