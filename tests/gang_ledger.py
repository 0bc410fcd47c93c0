"""Checker for pe_release_gangs / pe_assume_gangs and the inputs their CPU and GPU tests share.

The rule (include/placement.h): the gangs are placed gangs in the shape the placement calls take and return.  Every
pod slot whose node n is >= 0 and not a removed slot gives its group's request back to n (release) or takes it off n
(assume), in all four dimensions.  The call is all-or-nothing: in the dimensions a slot moves, a release may not
raise the residual above the reset snapshot and an assume may not lower it below 0; the first slot, in input order,
at which that happens names the refusal's node, and then nothing changes.

    apply(op, ...)        the rule, one pod slot at a time in Python integers over (residuals, snapshot, removed)
    release / assume      apply with the operation named
    Book                  residuals, snapshot and removed flags walked beside an engine through loads, node updates,
                          resets, placements, releases and assumes
    greedy_placement, domain_placement, first_fit_placement
                          real placements by the existing CPU checkers (the C oracle greedy, domain_placement.place,
                          first_fit.place_first_fit)
"""
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

import domain_placement as DP
import first_fit as FF
import oracle
from placement import synth

RELEASE, ASSUME = "release", "assume"
GiB = DP.GiB


class Outcome(NamedTuple):
    res: Optional[np.ndarray]      # int64 [4][N] after the call; None when it is refused
    pods: int                      # pod slots that counted; -1 when refused
    node: int                      # the refusal's node; -1 when the call goes through


@dataclass
class Gangs:
    """Placed gangs: a batch's job_group_off, group_count and group_req with the pod slots a placement returned."""
    group_off: np.ndarray      # int32 [V + 1]
    group_count: np.ndarray    # int32 [VG]
    group_req: np.ndarray      # int64 [VG][4]
    pod_node: np.ndarray       # int32 [sum of counts]: global node id per pod slot, -1 = skipped

    def arrays(self):
        return self.group_off, self.group_count, self.group_req, self.pod_node

    def __len__(self):
        return len(self.group_off) - 1

    def only(self, gangs):
        """The listed gangs, in the listed order, as Gangs of their own."""
        poff = DP.pod_offsets(self.group_count)
        off, cnt, req, pods = [0], [], [], []
        for v in gangs:
            for g in range(int(self.group_off[v]), int(self.group_off[v + 1])):
                cnt.append(int(self.group_count[g]))
                req.append([int(x) for x in self.group_req[g]])
                pods.extend(int(x) for x in self.pod_node[poff[g]:poff[g + 1]])
            off.append(len(cnt))
        return make_gangs_arrays(off, cnt, req, pods)

    def touched(self):
        """The distinct nodes >= 0 of the pod slots."""
        p = np.asarray(self.pod_node)
        return np.unique(p[p >= 0])


def make_gangs_arrays(off, cnt, req, pods):
    return Gangs(np.array(off, dtype=np.int32), np.array(cnt, dtype=np.int32), np.array(req, dtype=np.int64).reshape(-1, 4),
                 np.array(pods, dtype=np.int32))


def make_gangs(gangs):
    """Gangs of [[(request[4], [node per pod slot]), ...], ...]."""
    off, cnt, req, pods = [0], [], [], []
    for groups in gangs:
        for q, nodes in groups:
            cnt.append(len(nodes))
            req.append(q)
            pods.extend(nodes)
        off.append(len(cnt))
    return make_gangs_arrays(off, cnt, req, pods)


def of_batch(batch, pods):
    """The gangs of a placement call: its batch and the pod slots it returned."""
    return Gangs(np.asarray(batch.job_group_off, dtype=np.int32), np.asarray(batch.group_count, dtype=np.int32),
                 np.asarray(batch.group_req, dtype=np.int64).reshape(-1, 4), np.asarray(pods, dtype=np.int32))


# ---------------------------------------------------------------- the rule

def apply(op, res, snap, removed, gangs):
    """Outcome of one call, slot by slot in Python integers.  res, snap: [4][N]; removed: bool [N]."""
    assert op in (RELEASE, ASSUME)
    res = np.asarray(res)
    now = {}                                                # touched node -> its four residuals
    pods, s = 0, 0
    for g in range(int(gangs.group_off[-1])):
        q = [int(x) for x in gangs.group_req[g]]
        for _ in range(int(gangs.group_count[g])):
            n = int(gangs.pod_node[s])
            s += 1
            if n < 0 or removed[n]:
                continue
            r = now.setdefault(n, [int(res[d][n]) for d in range(4)])
            for d in range(4):
                if q[d] == 0:
                    continue                                # a dimension the slot does not move is not looked at
                r[d] += q[d] if op == RELEASE else -q[d]
                if (r[d] > int(snap[d][n])) if op == RELEASE else (r[d] < 0):
                    return Outcome(None, -1, n)
            pods += 1
    out = np.array(res, dtype=np.int64, copy=True)
    for n, r in now.items():
        out[:, n] = r
    return Outcome(out, pods, -1)


def release(res, snap, removed, gangs):
    return apply(RELEASE, res, snap, removed, gangs)


def assume(res, snap, removed, gangs):
    return apply(ASSUME, res, snap, removed, gangs)


class Book:
    """(residuals, snapshot, removed flags) of the GLOBAL inventory, walked beside an engine."""

    def __init__(self, cap, used):
        self.load(cap, used)

    def load(self, cap, used):
        self.snap = np.asarray(cap, dtype=np.int64) - np.asarray(used, dtype=np.int64)
        self.res = self.snap.copy()
        self.removed = np.zeros(self.snap.shape[1], dtype=bool)

    def reset(self):
        self.res = self.snap.copy()

    def node_set(self, n, cap4, used4):
        self.res[:, n] = self.snap[:, n] = np.asarray(cap4, dtype=np.int64) - np.asarray(used4, dtype=np.int64)
        self.removed[n] = False

    def node_remove(self, n):
        self.removed[n] = True

    def placed(self, res_after):
        """A placement call left these residuals (removed slots keep what the book holds)."""
        keep = self.removed
        self.res = np.where(keep[None, :], self.res, np.asarray(res_after, dtype=np.int64))

    def apply(self, op, gangs):
        out = apply(op, self.res, self.snap, self.removed, gangs)
        if out.node < 0:
            self.res = out.res
        return out

    def visible(self):
        """What pe_read_residuals shows: INT64_MIN on removed slots."""
        return np.where(self.removed[None, :], np.iinfo(np.int64).min, self.res)


# ---------------------------------------------------------------- real placements by the CPU checkers

@dataclass
class Placement:
    cap: np.ndarray
    used: np.ndarray
    labels: np.ndarray
    island: np.ndarray
    batch: synth.JobBatch
    pods: np.ndarray
    status: np.ndarray
    res_after: np.ndarray
    extra: tuple = ()          # what the placement call takes beyond the batch

    def residual(self):
        return self.cap - self.used

    def gangs(self):
        return of_batch(self.batch, self.pods)

    def book(self):
        return Book(self.cap, self.used)


def greedy_placement(n, seed=7, n_jobs=40, mix="mixed"):
    """The synth inventory of n nodes and a job mix placed by the C oracle greedy (pe_place_greedy's rule)."""
    inv = synth.make_inventory(n, seed)
    b = synth.make_jobs(n_jobs, seed, mix)
    pods, st, res = oracle.place_greedy(inv.residual(), inv.labels, b.job_group_off, b.priority, b.group_count, b.group_req,
                                        b.group_need)
    return Placement(inv.cap, inv.used, inv.labels, inv.island, b, pods, st, res)


def domain_placement(name, n, level=0):
    """A named hierarchy with its job mix placed by domain_placement.place (pe_place_greedy_domains' rule)."""
    c = DP.tree_case(name, n, level)
    pods, st, res = DP.place(c.residual(), c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent)
    return Placement(c.cap, c.used, c.labels, c.island, c.batch, pods, st, res, (c.job_domain, c.level, c.level_size, c.parent))


def first_fit_placement(name, n, level=0):
    """The same hierarchy with first_fit's pairs placed by first_fit.place_first_fit (pe_place_first_fit_domains)."""
    c, pj, pd = FF.pairs_case(name, n, level)
    pods, st, _, res = FF.place_first_fit(c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)
    return Placement(c.cap, c.used, c.labels, c.island, c.batch, pods, st, res, (pj, pd, c.level, c.level_size, c.parent))


def spread_gangs(nodes, req, per_gang=7):
    """One pod of `req` on every listed node, dealt over gangs of at most per_gang pods in one group each."""
    nodes = [int(x) for x in nodes]
    return make_gangs([[(list(req), nodes[i:i + per_gang])] for i in range(0, len(nodes), per_gang)])


def check_engine(eng, book, op, gangs, lo=None, hi=None):
    """Run the call on the engine, compare the pod count and every residual cell of the engine's shard ([lo, hi) of
    the book, default all of it) with the checker, and move the book on.  The checker must let the call through."""
    want = book.apply(op, gangs)
    assert want.node < 0, ("the checker refuses the call at node", want.node)
    got = (eng.release_gangs if op == RELEASE else eng.assume_gangs)(*gangs.arrays())
    assert got == want.pods, (got, want.pods)
    mine = book.visible()[:, lo:hi]
    back = eng.read_residuals()
    assert np.array_equal(back, mine), np.argwhere(back != mine)[:10].tolist()
    return want
