"""The domain calls' shared decision at its arithmetic edges: inventories, jobs and CPU-side restatements.  No
engine here: test_decision_edges_cpu.py checks on the CPU that the cases show what they are built to show and that
every wrong variant below changes an answer; test_gpu_decision_edges.py runs the five domain calls over them.

The five calls (pe_place_greedy_domains, pe_gang_fit_domains, pe_place_first_fit_domains, pe_gang_preempt_domains,
pe_place_min_member_domains) share node_key (pe_node_key.h), place_decide / take_of / place_take / island_request
(pe_place_step.h) and place_rollback (pe_place_job.h).  synth's inventories never reach the lines of that code:
memory and ephemeral quantities are multiples of 2^26, no score term saturates.  Here every job is AIMED at a line.

The inventory (edge_case): one level of three domains -- SMALL (window_lists.threshold_nodes(64) plus the arenas
below, well under PL_LDS_NODES = 1016: the instance with its state in LDS), LARGE (the same rows padded with plain
threshold nodes to exactly 1017, the smallest segment the global-memory instance takes) and EMPTY (no node).
threshold_nodes brings nodes on both sides of every saturation line of the key, in low-bit copies, and four
over-committed nodes (one residual -1).  An ARENA is a handful of hand-made nodes that share one label bit no other
node carries; the job aimed at it needs that bit, so its decisions are among those nodes alone, whatever the jobs
before it did elsewhere.  Arena jobs come first by priority; the roaming jobs (no need bit: every node of the
domain competes, window_lists.threshold_batch's among them) follow.  `used` is non-zero on every third node that
has room for it, so the residual is a real cap - used.

The lines, and the arena or roaming job aimed at each (ARENAS / edge_jobs have the numbers):
  low20, low24     requests with odd low 20 / 24 bits against nodes with low bits: (r - q) >> 20 borrows where
                   (r >> 20) - (q >> 20) does not, and the winner changes
  sat_tie          left0 = SMAX + 1 (lower id) against left0 = SMAX (higher id): both saturate, the lower id wins
  below_sat        scores SMAX (lower id) and SMAX - 1 out of four unsaturated terms: SMAX - 1 wins
  gpu_2^20         left2 = 2^20 (saturates, lower id) against left2 = 2^20 - 1 (2^40 - 2^20 + 5: wins)
  gpu_wrap         left2 = 2^44, whose << 20 leaves 64 bits, against a modest node, which wins
  take_d0 .. d3    a take bounded by each dimension in turn, the rest of the group on a second node bounded by
                   `left`; the residuals sit at k q - 1 and k q for a small q (1000, 2) and a large one (past 2^32)
  take_sat         a take of 3 from a node whose key is saturated for every pod of it (ties by id stay tied)
  take_2^32        floor(r / q) = 2^32 + 3 with left = 10: a quotient cut to 32 bits takes 3
  zero             the all-zero request: the take is `left`
  isl_exact        7 x ((2^63 - 1) / 7) = 2^63 - 1 exactly, on the all-INT64_MAX node (saturated afterwards);
  isl_overflow     the same request plus 1: refused; isl_none: 3 x 2^61 fits int64 and no node;
  isl_sat          an island unit on a saturated node
  rb, rb_after     a job that takes 3 and 2 pods on two nodes (3 x q1 is past 2^32) and then fails; the next job by
                   priority asks for the first node's whole memory: it fits only if all of it came back
  rbi, rbi_after   the same with the failure an island product that overflows
  need             a need bit that only some threshold nodes carry; the best-scoring node lacks it

place_take_many is the device's algorithm in Python integers: per decision the argmin key, then
t = min(left, min over q_d > 0 of r_d // q_d), or the island unit; it returns place_python's tuple plus what failed
and one record per decision.  Its key, take, island product and rollback product can be swapped for the WRONG
VARIANTS a device could implement and the old cases (synth inventories) could not tell from the rule:
  shift_first   (r1 >> 20) - (q1 >> 20), likewise >> 24            (KEYS)
  sat_2^40      saturation at 2^40, not 2^40 - 1                   (KEYS)
  gpu_wrap      left2 << 20 wrapped at 64 bits, unchecked          (KEYS)
  take_32       the take's quotients cut to 32 bits                (TAKES; a zero take would spin on the device:
                                                                    SPIN is its answer here)
  island_wrap   the island product wrapped to int64, not refused   (ISLANDS)
  rollback_32   the rollback's t x q_d in 32 bits                  (BACKS)
Not variants, because they are the same rule unless something wraps: dropping the per-term saturation (the sum of
four terms below 2^62 saturates whenever a term does) and `>` for `>=` at 2^20 GPUs (2^20 << 20 = 2^40 > SMAX
either way).  A signed division in the take is not one either: the take divides residuals and requests that are
both non-negative int64 (the node fits one pod), where signed and unsigned division agree -- no input differs.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import domain_placement as DP
import first_fit as FF
import gang_preempt as GP
import min_member as MM
import window_lists as WL
from oracle import semantics as S
from placement import synth

SMAX = WL.SMAX
INT64_MAX = WL.INT64_MAX
LO1, LO3 = WL.LO1, WL.LO3
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ISLAND, NO_LABEL = DP.ISLAND, DP.NO_LABEL
SMALL, LARGE, EMPTY = 0, 1, 2
LDS = 1016                                  # pe_kernels.h PL_LDS_NODES
N_LARGE = LDS + 1
ODD1, ODD3 = 0x5A5A5, 0xA5A5A5              # odd low 20 / 24 bits
Q7 = INT64_MAX // 7                         # 7 x Q7 = 2^63 - 1
QBIG = (5 << 32) | 0x12345                  # a memory request past 2^32
QEPH = (3 << 33) | 0xABCDEF                 # an ephemeral request past 2^32
Q_BELOW = (1000, (1 << 30) | ODD1, 1, (1 << 30) | ODD3)
Q_T0 = (1000, (1 << 20) + 3, 1, (1 << 24) + 5)
Q_SAT = (1000, (1 << 30) | ODD1, 0, 0)
SPIN = "a zero take: the device would spin"


def _plus(left, q):
    return tuple(a + b for a, b in zip(left, q))


_TOP = (2 ** 37 - 1, (2 ** 38 << 20) | 7, 2 ** 19, (2 ** 37 << 24) | 9)      # terms 2^37 - 1, 2^38, 2^39, 2^37: SMAX

# name -> the arena's nodes in id order (residuals); the arena's label bit is its position in this table
ARENAS = {
    "low20": [(12, 100 << 20, 0, 0), (12, (99 << 20) | LO1, 0, 0)],
    "low24": [(12, 0, 0, 100 << 24), (12, 0, 0, (99 << 24) | LO3)],
    "sat_tie": [(SMAX + 1 + 1000, 0, 0, 0), (SMAX + 1000, 0, 0, 0)],
    "below_sat": [_plus(_TOP, Q_BELOW), _plus((_TOP[0] - 1,) + _TOP[1:], Q_BELOW)],
    "gpu_2^20": [(1, 0, 2 ** 20 + 1, 0), (6, 0, 2 ** 20, 0)],
    "gpu_wrap": [(1, 0, 2 ** 44 + 1, 0), (5001, 0, 4, 0)],
    "take_d0": [(5 * 1000 - 1, 100 * Q_T0[1], 100, 100 * Q_T0[3]), (10 ** 6, 1000 * Q_T0[1], 1000, 1000 * Q_T0[3])],
    "take_d1": [(50, 3 * QBIG, 0, 0), (100_000, 2 * QBIG + 17, 0, 0)],
    "take_d2": [(100, 100 << 20, 6, 0), (100_000, 1000 << 20, 100, 0)],
    "take_d3": [(0, 0, 0, 4 * QEPH - 1), (5, 0, 0, 50 * QEPH)],
    "take_sat": [(2 ** 50, 3 * Q_SAT[1] + 5, 0, 0), (2 ** 50, 100 * Q_SAT[1], 0, 0)],
    "take_2^32": [(1000 * (2 ** 32 + 3) + 1, 0, 0, 0), (2 ** 60, 0, 0, 0)],
    "isl_none": [(1000, 0, 0, 0), (2 ** 61, 0, 0, 0)],
    "isl_sat": [(2 ** 50, 0, 0, 0), (2 ** 50, 0, 0, 0)],
    "rb": [(50, 3 * QBIG + 7, 0, 0), (100_000, 2 * QBIG + 17, 0, 0)],
    "rbi": [(4000, 0, 0, 0), (5000, 0, 0, 0)],
}
_BITS = [b for b in range(4, 31) if b != 20]                # bits 0, 1: threshold_nodes'; 20: NO_LABEL; 31: island
BIT = {name: 1 << _BITS[i] for i, name in enumerate(list(ARENAS) + ["need"])}
NEED_LINES = ("r2=2^20-1", "S=SMAX-1", "r3=INT64_MAX")       # the threshold lines whose nodes carry BIT["need"]


def edge_jobs(domain, zero_count=40):
    """[(name, domain, priority, [(count, request, need), ...])]: the jobs aimed at `domain`, arena jobs first."""
    b = BIT
    named = [
        ("low20", [(2, (1, (5 << 20) | ODD1, 0, 0), b["low20"])]),
        ("low24", [(2, (1, 0, 0, (5 << 24) | ODD3), b["low24"])]),
        ("sat_tie", [(1, (1000, 0, 0, 0), b["sat_tie"])]),
        ("below_sat", [(1, Q_BELOW, b["below_sat"])]),
        ("gpu_2^20", [(1, (1, 0, 1, 0), b["gpu_2^20"])]),
        ("gpu_wrap", [(1, (1, 0, 1, 0), b["gpu_wrap"])]),
        ("take_d0", [(10, Q_T0, b["take_d0"])]),
        ("take_d1", [(5, (10, QBIG, 0, 0), b["take_d1"])]),
        ("take_d2", [(5, (10, 1 << 20, 2, 0), b["take_d2"])]),
        ("take_d3", [(5, (0, 0, 0, QEPH), b["take_d3"])]),
        ("take_sat", [(5, Q_SAT, b["take_sat"])]),
        ("take_2^32", [(10, (1000, 0, 0, 0), b["take_2^32"])]),
        ("isl_exact", [(7, (Q7, 0, 0, Q7), ISLAND)]),
        ("isl_overflow", [(7, (Q7 + 1, 0, 0, 0), ISLAND)]),
        ("isl_none", [(3, (2 ** 61, 0, 0, 0), ISLAND | b["isl_none"])]),
        ("isl_sat", [(4, (1000, 0, 0, 0), ISLAND | b["isl_sat"])]),
        ("rb", [(5, (10, QBIG, 0, 0), b["rb"]), (1, (1, 0, 0, 0), NO_LABEL)]),
        ("rb_after", [(1, (50, 3 * QBIG + 7, 0, 0), b["rb"])]),
        ("rbi", [(6, (1000, 0, 0, 0), b["rbi"]), (3, (2 ** 62, 0, 0, 0), ISLAND)]),
        ("rbi_after", [(1, (4500, 0, 0, 0), b["rbi"])]),
        ("zero", [(zero_count, (0, 0, 0, 0), 0)]),
        ("need", [(2, (500, (1 << 30) | ODD1, 0, 0), b["need"])]),
    ]
    tb = WL.threshold_batch()
    named += [("threshold%d" % g, [(int(tb.group_count[g]), tuple(int(x) for x in tb.group_req[g]), int(tb.group_need[g]))])
              for g in range(len(tb.group_count))]
    return [(name, domain, 200 - i, groups) for i, (name, groups) in enumerate(named)]


@dataclass
class EdgeCase:
    case: DP.Case
    node_tag: list            # per node: the arena or threshold line it belongs to, None for a plain node
    job_name: list            # per job: edge_jobs' name
    min_member: object = None
    extra: dict = field(default_factory=dict)

    def jobs_named(self, name, domain=None):
        return [j for j, n in enumerate(self.job_name)
                if n == name and (domain is None or int(self.case.job_domain[j]) == domain)]


def edge_inventory():
    """(cap, used, labels as the engine keeps them, island, node_tag): SMALL's nodes, three nodes in no domain,
    LARGE's nodes."""
    cap, used, labels, island, tag = _edge_inventory()
    return cap.copy(), used.copy(), labels.copy(), island.copy(), list(tag)


@functools.lru_cache(maxsize=None)
def _edge_inventory():
    arena = [(name, r) for name, rows in ARENAS.items() for r in rows]
    res, lab, isl, tag = [], [], [], []
    for dom, n in ((SMALL, 64), (None, 3), (LARGE, N_LARGE - len(arena))):
        inv, tags = WL.threshold_nodes(max(n, 64))
        r = (inv.cap - inv.used)[:, :n] if dom is None else inv.cap - inv.used
        for i in range(r.shape[1]):
            t = None if dom is None or tags[i] is None else tags[i][0]
            res.append(tuple(int(x) for x in r[:, i]))
            bits = 0b11 if (t is not None or i % 5) else 0b10        # every fifth plain node lacks label bit 0
            lab.append(bits | (BIT["need"] if t in NEED_LINES and i % 2 == 0 else 0))
            isl.append(-1 if dom is None else dom)
            tag.append(t)
        if dom is not None:
            for name, row in arena:
                res.append(row)
                lab.append(0b11 | BIT[name])
                isl.append(dom)
                tag.append(name)
    r = np.array(res, dtype=object).T
    used = np.zeros(r.shape, dtype=object)
    for i in range(r.shape[1]):
        if min(r[:, i]) < 0:
            used[:, i] = [1 if v < 0 else 0 for v in r[:, i]]        # over-committed: 0 of 1 used
        elif i % 3 == 0 and max(r[:, i]) < INT64_MAX - (1 << 40):
            used[:, i] = [7 + i, (1 << 20) | i, 1, 3]
    cap = (np.maximum(r, 0) + np.where(r >= 0, used, 0)).astype(np.int64)
    used = used.astype(np.int64)
    assert np.array_equal((cap - used).astype(object), r) and (cap >= 0).all() and (used >= 0).all()
    island = np.array(isl, dtype=np.int32)
    assert int((island == SMALL).sum()) < LDS // 4 and int((island == LARGE).sum()) == N_LARGE
    return cap, used, synth.island_labels(np.array(lab, dtype=np.uint32), island), island, tag


def edge_case(zero_count=40, jobs=None):
    """The edge inventory with the edge batch for SMALL and LARGE and three jobs in EMPTY.  zero_count: the pods of
    the zero-request group, or (SMALL's, LARGE's)."""
    cap, used, labels, island, tag = edge_inventory()
    if jobs is None:
        zs, zl = zero_count if isinstance(zero_count, tuple) else (zero_count, zero_count)
        jobs = edge_jobs(SMALL, zs) + edge_jobs(LARGE, zl) + [
            ("empty_pod", EMPTY, 5, [(2, (0, 0, 0, 0), 0)]), ("empty_none", EMPTY, 5, [(0, Q_SAT, 0)]),
            ("empty_island", EMPTY, 4, [(7, (Q7, 0, 0, 0), ISLAND)])]
    batch, job_domain = DP.make_batch([(d, p, g) for _, d, p, g in jobs])
    return EdgeCase(DP.Case(cap, used, labels, island, [3], None, 0, batch, job_domain), tag, [n for n, _, _, _ in jobs])


def args_of(case, res=None):
    return (case.residual() if res is None else res, case.labels, case.island, case.batch, case.job_domain, case.level,
            case.level_size, case.parent)


# ---------------------------------------------------------------- the rule's pieces and their wrong variants

def _key_of(score):
    def key(res4, labels, q4, need, node):
        if (labels & need) != need:
            return None
        left = [int(r) - int(q) for r, q in zip(res4, q4)]
        if any(v < 0 for v in left):
            return None
        return (score(left, res4, q4) << 24) | node
    return key


def _shift_first(left, r, q):
    terms = [left[0], (r[1] >> 20) - (q[1] >> 20), left[2] << 20, (r[3] >> 24) - (q[3] >> 24)]
    return min(SMAX, sum(min(SMAX, t) for t in terms))


def _sat_2_40(left, r, q):
    terms = [left[0], left[1] >> 20, left[2] << 20, left[3] >> 24]
    return min(1 << 40, sum(min(1 << 40, t) for t in terms))


def _gpu_wrap(left, r, q):
    a, b, c, d = left[0], left[1] >> 20, (left[2] << 20) & M64, left[3] >> 24
    s = (a + b + c + d) & M64
    return SMAX if a > SMAX or b > SMAX or d > SMAX or s > SMAX else s


KEYS = {"shift_first": _key_of(_shift_first), "sat_2^40": _key_of(_sat_2_40), "gpu_wrap": _key_of(_gpu_wrap)}


def take_rule(r4, q4, left):
    """(t, bound, smallest quotient or None): bound is the first dimension whose quotient is below `left`."""
    quot = [r // q if q > 0 else None for r, q in zip(r4, q4)]
    have = [v for v in quot if v is not None]
    if not have or min(have) >= left:
        return left, "left", min(have) if have else None
    return min(have), quot.index(min(have)), min(have)


def _take_32(r4, q4, left):
    quot = [(r // q) & M32 if q > 0 else None for r, q in zip(r4, q4)]
    have = [v for v in quot if v is not None]
    if not have or min(have) >= left:
        return left, "left", min(have) if have else None
    return min(have), quot.index(min(have)), min(have)


def island_rule(q4, count):
    s = [int(x) * count for x in q4]
    return s if all(v <= INT64_MAX for v in s) else None


def _island_wrap(q4, count):
    return [((int(x) * count + (1 << 63)) & M64) - (1 << 63) for x in q4]


def back_rule(t, q):
    return t * q


def _back_32(t, q):
    return (t * q) & M32


TAKES, ISLANDS, BACKS = {"take_32": _take_32}, {"island_wrap": _island_wrap}, {"rollback_32": _back_32}
VARIANTS = dict([(k, {"key": v}) for k, v in KEYS.items()] + [(k, {"take": v}) for k, v in TAKES.items()] +
                [(k, {"island": v}) for k, v in ISLANDS.items()] + [(k, {"back": v}) for k, v in BACKS.items()])


def _terms(left):
    return [left[0], left[1] >> 20, left[2] << 20, left[3] >> 24]


def place_take_many(res, labels, island, batch, job_domain, level, level_size, parent, key=S.appendix_b_key,
                    take=take_rule, island_req=island_rule, back=back_rule, watch=None):
    """The device's algorithm in Python integers.  Returns (pods, status, residual [4][N], rollbacks, fails, records):
    the first four as domain_placement.place_python; fails = [(job, group, "overflow" | "no_node")]; one record per
    decision: job, group, node, take, bound (a dimension, "left" or "unit"), quot (the smallest quotient), left, q
    (the request scored), r (the winner's residuals before), sat_before / sat_after (the key of the take's first
    and last pod saturated), runner (the node of the second smallest key, its residuals in runner_r) and -- with
    watch = {name: key function} -- wrong (the names whose argmin is another node) and need_best (the node that
    wins once the need's label bits are ignored).  A take of 0 ends the run with SPIN for an answer."""
    R = [[int(x) for x in row] for row in res]
    dom = DP.dom_level(island, level, level_size, parent)
    members = {}
    for n, d in enumerate(dom):
        members.setdefault(int(d), []).append(n)
    J = len(batch.priority)
    poff = DP.pod_offsets(batch.group_count)
    pods, status = [-1] * poff[-1], [0] * J
    rollbacks, fails, records = [], [], []
    lab = [int(x) for x in labels]

    def ranked(cands, q, need, kf):
        keys = sorted(k for k in (kf([R[d][n] for d in range(4)], lab[n], q, need, n) for n in cands) if k is not None)
        return keys[:2]

    for j in sorted(range(J), key=lambda j: (-int(batch.priority[j]), j)):
        cands = members.get(int(job_domain[j]), [])
        log, ok = [], True
        for g in range(int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])):
            q = [int(x) for x in batch.group_req[g]]
            need, left = int(batch.group_need[g]), int(batch.group_count[g])
            if left <= 0:
                continue
            unit = bool(need & ISLAND)
            s = q
            if unit:
                s = island_req(q, left)
                if s is None:
                    fails.append((j, g, "overflow"))
                    ok = False
                    break
            slot = poff[g]
            while left > 0:
                mine = [n for n in cands if (lab[n] & need) == need]
                best = ranked(mine, s, need, key)
                if not best:
                    fails.append((j, g, "no_node"))
                    ok = False
                    break
                n = best[0] & 0xFFFFFF
                r = [R[d][n] for d in range(4)]
                t, bound, quot = (left, "unit", None) if unit else take(r, s, left)
                if t <= 0:
                    return SPIN, SPIN, SPIN, rollbacks, fails, records
                last = r if unit else [r[d] - (t - 1) * s[d] for d in range(4)]
                rec = dict(job=j, group=g, node=n, take=t, bound=bound, quot=quot, left=left, q=list(s), r=r,
                           sat_before=best[0] >> 24 == SMAX,
                           sat_after=(key(last, lab[n], s, need, n) or 0) >> 24 == SMAX,
                           runner=best[1] & 0xFFFFFF if len(best) > 1 else None)
                rec["runner_r"] = None if rec["runner"] is None else [R[d][rec["runner"]] for d in range(4)]
                if watch is not None:
                    rec["wrong"] = {name for name, kf in watch.items() if (ranked(mine, s, need, kf)[0] & 0xFFFFFF) != n}
                    every = ranked(cands, s, need & ISLAND, key)
                    rec["need_best"] = every[0] & 0xFFFFFF if every else None
                records.append(rec)
                m = 1 if unit else t
                for d in range(4):
                    R[d][n] -= m * s[d]
                log.append((n, g, t))
                pods[slot:slot + t] = [n] * t
                slot += t
                left -= t
            if not ok:
                break
        if not ok:
            for n, g, t in log:
                for d in range(4):
                    R[d][n] += back(t, int(batch.group_req[g][d]))
            p0, p1 = poff[int(batch.job_group_off[j])], poff[int(batch.job_group_off[j + 1])]
            pods[p0:p1] = [-1] * (p1 - p0)
            status[j] = 1
            rollbacks.append((j, [n for n, _, _ in log]))
    return pods, status, R, rollbacks, fails, records


# ---------------------------------------------------------------- what the cases must show

ITEMS = ("low20", "low24", "sat_tie", "below_sat", "gpu_2^20", "gpu_wrap", "take_saturated", "take_dim0", "take_dim1",
         "take_dim2", "take_dim3", "take_left", "kq-1_small", "kq_small", "kq-1_large", "kq_large", "quotient_2^32",
         "zero_request", "island_exact", "island_overflow", "island_no_node", "island_saturated", "rollback_big",
         "rollback_reused", "rollback_island_overflow", "need")


def items_shown(ec, answer, domain):
    """{item: shown} for the decisions of `domain` in place_take_many(..., watch=KEYS)'s answer."""
    c, b = ec.case, ec.case.batch
    pods, status, _, rollbacks, fails, records = answer
    recs = [r for r in records if int(c.job_domain[r["job"]]) == domain]
    mine = lambda j: int(c.job_domain[j]) == domain
    lab = [int(x) for x in c.labels]

    def left(r, q):
        return [a - v for a, v in zip(r, q)]

    def pair(r, test):
        return r["runner"] is not None and test(left(r["r"], r["q"]), left(r["runner_r"], r["q"]), r)

    def kq(r, off, large):
        d = r["bound"]
        return isinstance(d, int) and r["r"][d] == (r["take"] + off) * r["q"][d] - off and \
            (r["q"][d] > M32 if large else r["q"][d] < 1 << 16)

    out = dict.fromkeys(ITEMS, False)
    for r in recs:
        q, w = r["q"], r.get("wrong", ())
        out["low20"] |= "shift_first" in w and q[1] & 1 == 1 and q[3] & LO3 == 0
        out["low24"] |= "shift_first" in w and q[3] & 1 == 1 and q[1] & LO1 == 0
        out["sat_tie"] |= "sat_2^40" in w and pair(r, lambda a, x, r: a[0] == SMAX + 1 and x[0] == SMAX and r["runner"] > r["node"])
        out["below_sat"] |= pair(r, lambda a, x, r: sum(_terms(a)) == SMAX - 1 and sum(_terms(x)) == SMAX and
                                 min(_terms(a) + _terms(x)) > 0 and r["runner"] < r["node"])
        out["gpu_2^20"] |= pair(r, lambda a, x, r: a[2] == 2 ** 20 - 1 and x[2] == 2 ** 20 and r["runner"] < r["node"])
        out["gpu_wrap"] |= "gpu_wrap" in w and pair(r, lambda a, x, r: x[2] >= 2 ** 44 and not r["sat_before"])
        out["take_saturated"] |= r["take"] >= 2 and r["bound"] != "unit" and r["sat_before"] and r["sat_after"]
        for d in range(4):
            out["take_dim%d" % d] |= r["bound"] == d and r["take"] >= 2
        out["take_left"] |= r["bound"] == "left" and r["take"] >= 2 and any(q)
        out["kq-1_small"] |= kq(r, 1, False)
        out["kq_small"] |= kq(r, 0, False)
        out["kq-1_large"] |= kq(r, 1, True)
        out["kq_large"] |= kq(r, 0, True)
        out["quotient_2^32"] |= r["quot"] is not None and r["quot"] > 1 << 32 and 0 < r["quot"] & M32 < r["left"] < r["quot"]
        out["zero_request"] |= not any(q) and r["bound"] == "left" and r["take"] == r["left"] >= 2
        out["island_exact"] |= r["bound"] == "unit" and INT64_MAX in q and ec.node_tag[r["node"]] == "all INT64_MAX"
        out["island_saturated"] |= r["bound"] == "unit" and r["sat_before"]
        nb = r.get("need_best")
        out["need"] |= bool(q and r["bound"] != "unit" and nb is not None and nb != r["node"] and
                            ec.node_tag[r["node"]] in NEED_LINES and
                            lab[nb] & int(b.group_need[r["group"]]) != int(b.group_need[r["group"]]))
    for j, g, why in fails:
        if mine(j):
            took = any(r["job"] == j for r in recs)
            isl = bool(int(b.group_need[g]) & ISLAND)
            out["island_overflow"] |= why == "overflow"
            out["island_no_node"] |= why == "no_node" and isl and island_rule(b.group_req[g], int(b.group_count[g])) is not None
            out["rollback_island_overflow"] |= why == "overflow" and took
    order = sorted((j for j in range(len(status)) if mine(j)), key=lambda j: (-int(b.priority[j]), j))
    for j, nodes in rollbacks:
        if not mine(j) or len(set(nodes)) < 2:
            continue
        took = [r for r in recs if r["job"] == j]
        big = any(r["take"] > 1 for r in took) and \
            any(ec.node_tag[r["node"]] is not None and max(r["take"] * v for v in r["q"]) > M32 for r in took)
        out["rollback_big"] |= big
        nxt = order[order.index(j) + 1] if order.index(j) + 1 < len(order) else None
        if big and nxt is not None and status[nxt] == 0:
            for r in (r for r in recs if r["job"] == nxt):       # it fits its node only with what came back
                held = [sum(x["take"] * x["q"][d] for x in took if x["node"] == r["node"]) for d in range(4)]
                out["rollback_reused"] |= any(r["r"][d] - held[d] < r["q"][d] for d in range(4))
    return out


def domain_answer(case, answer, domain):
    """The cells of `domain` in an answer's (pods, status, residual): what a variant must change."""
    pods, status, R = answer[0], answer[1], answer[2]
    if pods is SPIN or pods == SPIN:
        return SPIN
    poff = DP.pod_offsets(case.batch.group_count)
    jgo = case.batch.job_group_off
    jobs = [j for j in range(len(status)) if int(case.job_domain[j]) == domain]
    nodes = np.nonzero(np.asarray(case.island) == domain)[0]
    return ([list(pods[poff[int(jgo[j])]:poff[int(jgo[j + 1])]]) for j in jobs], [int(status[j]) for j in jobs],
            [[int(R[d][n]) for n in nodes] for d in range(4)])


# ---------------------------------------------------------------- the other four calls' inputs

def fit_pairs(ec):
    """(pair_job, pair_domain): every edge job with all three domains, SMALL first for SMALL's jobs, LARGE first
    for the others."""
    pj, pd = [], []
    for j, d in enumerate(ec.case.job_domain):
        for x in ([SMALL, EMPTY, LARGE] if int(d) != LARGE else [LARGE, EMPTY, SMALL]):
            pj.append(j)
            pd.append(x)
    return np.array(pj, dtype=np.int32), np.array(pd, dtype=np.int32)


def first_fit_case(zero_count=40):
    """(EdgeCase, pair_job, pair_domain): SMALL's edge jobs list [SMALL, LARGE], LARGE's list [LARGE, SMALL].  Added:
    two copies of `cross`, a job that takes a pod of the sat_tie arena and then the island unit of 2^63 - 1, both
    listing [SMALL, LARGE] -- the second finds the all-INT64_MAX node of SMALL taken, gives its first pod back
    (a rollback) and is placed in LARGE (before LARGE's own isl_exact, which then fails there); and `hopeless`,
    whose island product overflows in both."""
    cross = [(1, (1000, 0, 0, 0), BIT["sat_tie"]), (7, (Q7, 0, 0, Q7), ISLAND)]
    jobs = edge_jobs(SMALL, zero_count) + edge_jobs(LARGE, zero_count)
    jobs += [("cross", SMALL, 300, cross), ("cross", SMALL, 299, cross),
             ("hopeless", SMALL, 298, [(1, (1000, 0, 0, 0), BIT["sat_tie"]), (7, (Q7 + 1, 0, 0, 0), ISLAND)])]
    ec = edge_case(jobs=jobs)
    pj, pd = [], []
    for j, d in enumerate(ec.case.job_domain):
        pj += [j, j]
        pd += [int(d), LARGE + SMALL - int(d)]
    return ec, np.array(pj, dtype=np.int32), np.array(pd, dtype=np.int32)


def min_member_cases(zero_count=40):
    """{name: min_member.Case} over the edge batch: "all" (min_member = -1 everywhere: pe_place_greedy_domains'
    answer) and "partial" (take_sat's phase 1 is 3 pods: one take of 3 from the saturated node; the take_d* jobs are
    cut inside their first take, on its edge and one pod past it; rb keeps its failing group mandatory and rolls
    back; rbi's overflowing island group is optional: the job is placed in part)."""
    ec = edge_case(zero_count)
    c = ec.case
    J = len(ec.job_name)
    cut = {"take_sat": 3, "take_d0": 2, "take_d1": 3, "take_d2": 4, "take_d3": 1, "take_2^32": 4, "zero": 1, "rb": 6,
           "low20": 1, "isl_sat": 2, "rbi": 6, "need": 0}
    total = [int(c.batch.group_count[int(c.batch.job_group_off[j]):int(c.batch.job_group_off[j + 1])].sum()) for j in range(J)]
    partial = np.array([min(cut.get(ec.job_name[j], MM.ALL), total[j]) for j in range(J)], dtype=np.int32)
    mk = lambda mm: MM.Case(c.cap, c.used, c.labels, c.island, c.level_size, None, 0, c.batch, c.job_domain, mm)
    return ec, {"all": mk(np.full(J, MM.ALL, dtype=np.int32)), "partial": mk(partial)}


def preempt_case(zero_count=40):
    """(EdgeCase of the incoming jobs, gang_preempt.PCase, the resident job's name per victim): the residents are the
    gangs the edge batch placed (domain_placement.place), accounted in `used`; the incoming jobs are the edge jobs
    that the same batch, sent again, does not place: each is paired with its own domain and the victims that hold a
    pod there, in ascending priority after one stranger (gang_preempt.pair_lists).  The jobs that no release helps
    come first: they take the list lengths 0, 1, 2, 63 and 64 that pair_lists forces on the first pairs."""
    ec = edge_case(zero_count)
    c, b = ec.case, ec.case.batch
    pods, status, res = DP.place(*args_of(c))
    poff = DP.pod_offsets(b.group_count)
    vics, who = [], []
    for j in np.nonzero(status == 0)[0]:
        g0, g1 = int(b.job_group_off[j]), int(b.job_group_off[j + 1])
        if poff[g1] > poff[g0]:
            vics.append((int(b.priority[j]), [([int(x) for x in b.group_req[g]], pods[poff[g]:poff[g + 1]].tolist())
                                              for g in range(g0, g1)]))
            who.append(int(j))
    vic = GP.make_victims(vics)
    _, again, _ = DP.place(*args_of(c, res))
    keep = [int(j) for j in np.nonzero(again == 1)[0] if int(c.job_domain[j]) != EMPTY]
    keep.sort(key=lambda j: (status[j] == 0, j))             # the jobs that failed the first time too: hopeless
    jobs = [(ec.job_name[j], int(c.job_domain[j]), int(b.priority[j]),
             [(int(b.group_count[g]), [int(x) for x in b.group_req[g]], int(b.group_need[g]))
              for g in range(int(b.job_group_off[j]), int(b.job_group_off[j + 1]))]) for j in keep]
    batch, job_domain = DP.make_batch([(d, p, g) for _, d, p, g in jobs])
    case = DP.Case(c.cap, c.cap - res, c.labels, c.island, c.level_size, None, 0, batch, job_domain)
    pj = np.arange(len(jobs), dtype=np.int32)
    pvo, pv = GP.pair_lists(case, vic, pj, job_domain, seed=5)
    inc = EdgeCase(case, ec.node_tag, [n for n, _, _, _ in jobs])
    return inc, GP.PCase(case, vic, pj, job_domain.astype(np.int32), pvo, pv), [ec.job_name[j] for j in who]


def preempt_restores(inc, pc, answer):
    """Per pair whose job needs victims: (job name, domain, nodes that the final victims' release moves back across a
    line: onto a residual of k q_d for the job's request with k >= 2, or from an unsaturated zero-request key to a
    saturated one)."""
    c = pc.case
    dom = DP.dom_level(c.island, c.level, c.level_size, c.parent)
    pods_of = [pc.vic.pods(v) for v in range(len(pc.vic))]
    res = c.residual()
    out = []
    for p in range(len(pc.pair_job)):
        if answer[2][p] < 1:
            continue
        j, d = int(pc.pair_job[p]), int(pc.pair_domain[p])
        final = GP.final_set(pc.pair_vic_off, pc.pair_vic, p, answer[1][p])
        after = GP.released(res, dom, d, pods_of, final)
        q = [int(x) for x in c.batch.group_req[int(c.batch.job_group_off[j])]]
        nodes = []
        for n in np.nonzero((after != res).any(axis=0))[0]:
            a, r = [int(x) for x in after[:, n]], [int(x) for x in res[:, n]]
            kq = any(q[k] > 0 and a[k] % q[k] == 0 and a[k] // q[k] >= 2 and r[k] < q[k] for k in range(4))
            zero = [0, 0, 0, 0]
            sat = min(r) >= 0 and S.appendix_b_key(a, 0, zero, 0, 0) >> 24 == SMAX > S.appendix_b_key(r, 0, zero, 0, 0) >> 24
            if kq or sat:
                nodes.append((int(n), "kq" if kq else "saturation"))
        out.append((inc.job_name[j], d, nodes))
    return out


def first_fit_crossed(ec, pair_job, pair_domain, status, pair):
    """Whether one `cross` job stands in SMALL by its first pair and the other, which found the all-INT64_MAX node
    taken there after its own first group had taken a pod (the sat_tie arena holds many), stands in LARGE by its
    second pair."""
    first, second = ec.jobs_named("cross")
    cand = FF.candidates(pair_job, len(status))
    return bool(status[first] == 0 and pair[first] == cand[first][0] and int(pair_domain[pair[first]]) == SMALL and
                status[second] == 0 and pair[second] == cand[second][1] and int(pair_domain[pair[second]]) == LARGE)


def min_member_cut_on_saturated_take(ec, mc):
    """Whether some placed job with 0 < M < T ends its phase 1 (the batch at its mandatory counts) on a take of at
    least 2 from a node whose key is saturated for every pod of the take."""
    m, _, M, T = MM.shares(mc.batch, mc.min_member)
    b = mc.batch
    cut = synth.JobBatch(b.job_group_off, b.priority, np.array(m, dtype=np.int32), b.group_req, b.group_need, b.kind)
    _, status, _, _, _, records = place_take_many(mc.residual(), mc.labels, mc.island, cut, mc.job_domain, mc.level,
                                                   mc.level_size, mc.parent)
    for j in range(len(M)):
        mine = [r for r in records if r["job"] == j]
        if 0 < M[j] < T[j] and status[j] == 0 and mine:
            last = mine[-1]
            if last["take"] >= 2 and last["bound"] != "unit" and last["sat_before"] and last["sat_after"]:
                return True
    return False
