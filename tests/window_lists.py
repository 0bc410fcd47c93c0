"""The real engine's window lists: the script one context is walked through, the lists a window must hold, and the
reader of a PE_DUMP_WINDOWS file.  No engine here: test_gpu_window_lists.py walks engine contexts through the script
and compares the first window of every pe_place_greedy call with expected_lists(), test_cand_lists_cpu.py checks on
the host model alone that the script yields lists of every kind.

Every call of the script is at most one window (a handful of jobs), so the state its lists were scanned at is the
state before the call: the first window has no seeds and walks lists of the configured topk.  The contract
(cand_lists.py): the list is the min(K, |B|) smallest of B = the feasible keys below the bound, limit = the (K+1)-th or
the bound.  The bound is NO_KEY for the sorted walk; for the scan it is merge_kernel's G, the smallest wave bound --
a wave spans 1024 nodes, lane l holds nodes l, l + 64, ... of the span, the wave's bound is the smallest second-best
key of its lanes (scan_kernel), restated in scan_bound().

The script of one configuration (topk, nodes, inventory kind):
  load; place a; place b (no reset: call a's nodes are in the overlay); pe_update_nodes; place c; place d (gangs and
  groups that need a label no node carries: empty lists); reset; place a
Inventories: synth's random one; all nodes identical (ties by id, one dense cluster of consecutive keys); a mix with
saturating nodes (2^41 cpu, 2^61 memory, 2^21 gpus: evaluated in the overlay only) and over-committed ones (negative
residuals: in no list).

EDGE_CONFIGS walk the same script over inventories and requests with LOW BITS, which synth never draws (its memory
and ephemeral quantities are multiples of 2^26: lo20 / lo24 are 0 everywhere and no key ever borrows).  A node
carries K(n) = (S(n) << 24) | gid and a group's key on it is K(n) - ((s(q) + borrows) << 24), borrows =
[lo20(r1) < lo20(q1)] + [lo24(r3) < lo24(q3)] (pe_kernels.hip node_prep): the walk orders nodes by K(n), which is not
key order once borrows differ, so its stop bound subtracts the largest borrow count; fast_key carries borrows << 24
out of the low word exactly when (score + borrows) & 0xFF < borrows.
  plateau      long runs of equal S(n), random low bits: later rounds hold smaller keys than collected ones
  staircase    consecutive S through every residue mod 256, random low bits: the carry into the high word
  rare_borrow  one plateau, every 100th node borrows twice and the rest never: the K smallest keys are the first K
               rare nodes, a long walk through the in-walk compaction
  thresholds   hand-made nodes on both sides of every line of node_prep (threshold_nodes) and hand-made requests
               (threshold_batch): saturated s(q), KQ2, overlay-only groups
Their batches are synth's with random low bits added to the memory and ephemeral requests (low_bits), and the update
step's donor nodes carry odd low bits."""
import re
import struct
from collections import namedtuple

import numpy as np

import scan_emulator
from inventory_model import Model, make_deltas
from placement import synth

NO_KEY = (1 << 64) - 1
UNKNOWN_LABEL = np.uint32(1 << 20)
WINDOW_GROUPS, WINDOW_PODS = 112, 1024      # the engine's defaults
NODE_STATE_BYTES = 64                       # pe_resolver.h NodeState: one cache line per node

# engine modes: constructor arguments and environment
MODES = {
    "walk": ({}, {}),
    "walk_sequential": ({"greedy_flags": 1}, {}),
    "scan": ({"greedy_flags": 2}, {}),
    "scan_sequential": ({"greedy_flags": 3}, {}),
    "resort1": ({"resort_nodes": 1}, {}),
    "one_index": ({"resort_nodes": 1 << 30}, {}),
    "delayed_switch": ({"resort_nodes": 4}, {"PE_ASYNC_RESORT": "1", "PE_WALK_SWITCH_DELAY": "3"}),
}
SCAN_MODES = ("scan", "scan_sequential")

TOPK = (1, 2, 8, 256, 1023)
NODES = (1, 1023, 1024, 1025, 2049, 5000)
KINDS = ("random", "identical", "saturating")
Config = namedtuple("Config", "topk n kind")
CONFIGS = (Config(1, 1, "identical"), Config(2, 1023, "random"), Config(8, 1024, "saturating"),
           Config(256, 1025, "random"), Config(1023, 2049, "identical"), Config(256, 5000, "saturating"),
           Config(1023, 5000, "random"), Config(8, 5000, "identical"), Config(1023, 1023, "saturating"),
           Config(2, 2049, "random"), Config(1, 1025, "random"))

EDGE_KINDS = ("plateau", "staircase", "rare_borrow", "thresholds")
EDGE_CONFIGS = (Config(8, 5000, "plateau"), Config(256, 5000, "plateau"), Config(1023, 5000, "plateau"),
                Config(1023, 5000, "staircase"), Config(256, 2049, "staircase"), Config(256, 30_000, "rare_borrow"),
                Config(1023, 1023, "thresholds"), Config(8, 64, "thresholds"))
SMAX = (1 << 40) - 1
INT64_MAX = (1 << 63) - 1
LO1, LO3 = (1 << 20) - 1, (1 << 24) - 1     # the bits of memory / ephemeral storage that the score shifts out
RARE_EVERY = 100

Step = namedtuple("Step", "op arg")


def plain_inventory(res, used=None):
    """Nodes with the residuals res [4][N], labels 0b11 and an island each."""
    cap = np.ascontiguousarray(res, dtype=np.int64)
    island = np.arange(cap.shape[1], dtype=np.int32)
    labels = synth.island_labels(np.full(cap.shape[1], 0b11, np.uint32), island)
    return synth.Inventory(cap, np.zeros_like(cap) if used is None else used, labels, island)


def threshold_nodes(n):
    """(Inventory, tags): the nodes of kind "thresholds".  tags[i] = (line, class node_prep must give) for a
    hand-made node, None for a plain one.  Each line comes in a few copies that differ in the low bits only, two
    plain nodes after each line while they last, the rest of the plain nodes at the end."""
    m1, m3 = 512 * synth.GiB, 2 * synth.TiB
    lows = ((1, 1), (LO1, LO3), (0x80001, 0x7FFFFF))
    top = SMAX - 1 - (m1 >> 20) - (8 << 20) - (m3 >> 24)       # r0 of the node with S = SMAX - 1
    lines = [
        ("S=SMAX-1", "walk", [(top, m1 + a, 8, m3 + b) for a, b in lows]),
        ("S=SMAX", "slow", [(top + 1, m1 + a, 8, m3 + b) for a, b in lows]),
        ("r0=SMAX", "slow", [(SMAX, 0, 0, 0), (SMAX, LO1, 0, LO3)]),
        ("r0=SMAX+1", "slow", [(SMAX + 1, 0, 0, 0), (SMAX + 1, 1, 0, 1)]),
        ("r1=(SMAX-2)<<20|odd", "walk", [(0, (SMAX - 2) << 20 | a, 0, 0) for a, _ in lows]),
        ("r1=2^60-1", "slow", [(0, (1 << 60) - 1, 0, 0), (5, (1 << 60) - 1, 0, LO3)]),
        ("r1=2^60", "slow", [(0, 1 << 60, 0, 0), (5, (1 << 60) + 1, 0, 1)]),
        ("r2=2^20-1", "walk", [(1000, 64 * synth.GiB + a, (1 << 20) - 1, synth.TiB + b) for a, b in lows]),
        ("r2=2^20", "slow", [(1000, 64 * synth.GiB + a, 1 << 20, synth.TiB + b) for a, b in lows[:2]]),
        ("r3=INT64_MAX", "walk", [(1000, 64 * synth.GiB + a, 8, INT64_MAX) for a, _ in lows]),
        ("all INT64_MAX", "slow", [(INT64_MAX,) * 4]),
        ("all 0", "walk", [(0, 0, 0, 0)] * 2),
        ("one -1", "never", [tuple(-1 if e == d else v for e, v in enumerate((96_000, m1 + 1, 8, m3 + 1)))
                             for d in range(4)]),
    ]
    special = sum(len(c) for _, _, c in lines)
    assert n >= special + 2 * len(lines), n
    rng = np.random.default_rng(17)
    res, tags = [], []

    def plain(count):
        for _ in range(count):
            res.append((96_000 + len(res), m1 + int(rng.integers(0, 1 << 20)), 8, m3 + int(rng.integers(0, 1 << 24))))
            tags.append(None)

    for name, cls, copies in lines:
        for c in copies:
            res.append(c)
            tags.append((name, cls))
        plain(2)
    plain(n - len(res))
    r = np.array(res, dtype=np.int64).T
    return plain_inventory(np.maximum(r, 0), np.where(r < 0, 1, 0).astype(np.int64)), tags   # (-1 = 0 of 1 used)


def make_inventory(n, kind, seed=3):
    if kind in ("plateau", "staircase", "rare_borrow"):
        rng = np.random.default_rng(seed + 8)
        i = np.arange(n, dtype=np.int64)
        r = np.empty((4, n), dtype=np.int64)
        r[0] = {"plateau": 96_000 + i // 2500, "staircase": 96_000 + (7 * i) % 600, "rare_borrow": 96_000 + 0 * i}[kind]
        r[1] = 512 * synth.GiB + rng.integers(0, 1 << 20, n)
        r[2] = 8
        r[3] = 2 * synth.TiB + rng.integers(0, 1 << 24, n)
        if kind == "rare_borrow":       # every RARE_EVERY-th node borrows twice against any low bits, the rest never
            r[1] = 512 * synth.GiB + np.where(i % RARE_EVERY == 0, 0, LO1)
            r[3] = 2 * synth.TiB + np.where(i % RARE_EVERY == 0, 0, LO3)
        return plain_inventory(r)
    if kind == "thresholds":
        return threshold_nodes(n)[0]
    if kind == "random":
        return synth.make_inventory(n, seed, 0.3)
    if kind == "identical":
        cap = np.repeat(np.array([[128_000], [1 << 40], [8], [2 << 40]], dtype=np.int64), n, axis=1)
        island = np.arange(n, dtype=np.int32)
        return synth.Inventory(cap, np.zeros_like(cap), synth.island_labels(np.full(n, 0b11, np.uint32), island), island)
    inv = synth.make_inventory(n, seed + 1, 0.3)
    sat = np.arange(2, n, 5)
    inv.cap[0, sat], inv.cap[1, sat], inv.cap[2, sat] = 1 << 41, 1 << 61, 1 << 21
    inv.used[:, sat] = 0
    inv.labels[sat] |= 1
    over = np.arange(4, n, 7)
    inv.used[0, over] = inv.cap[0, over] + 500
    return inv


def batch(n_jobs, seed, mix="mixed"):
    return synth.make_jobs(n_jobs, seed, mix)


def batch_d(seed):
    """Whole-node gangs, and a mixed job whose last group needs a label no node carries."""
    a, b = synth.make_jobs(3, seed, "gang8"), synth.make_jobs(4, seed + 1, "mixed")
    off = np.concatenate([a.job_group_off, a.job_group_off[-1] + b.job_group_off[1:]]).astype(np.int32)
    out = synth.JobBatch(off, np.concatenate([a.priority, b.priority]), np.concatenate([a.group_count, b.group_count]),
                         np.concatenate([a.group_req, b.group_req]), np.concatenate([a.group_need, b.group_need]),
                         np.concatenate([a.kind, b.kind]))
    out.group_count[out.group_count == 0] = 1
    out.group_need[-1] |= UNKNOWN_LABEL
    out.group_need[int(off[4]) - 1] |= UNKNOWN_LABEL
    return out


def low_bits(b, seed, nonzero=False):
    """The batch with random low bits added to every memory and ephemeral request (nonzero: none of them 0)."""
    rng = np.random.default_rng(seed)
    G = len(b.group_count)
    b.group_req[:, 1] += rng.integers(0, 1 << 20, G) | int(nonzero)
    b.group_req[:, 3] += rng.integers(0, 1 << 24, G) | int(nonzero)
    return b


def threshold_batch(variant=0):
    """Single-group jobs at the edges of s(q) (walk_kernel's sq, KQ, KQ2) for the nodes of threshold_nodes.  variant 1:
    the last two groups need a label no node carries."""
    m1, m3 = 512 * synth.GiB, 2 * synth.TiB
    top = SMAX - 1 - (m1 >> 20) - (8 << 20) - (m3 >> 24)
    isl = int(synth.LABEL_ISLAND)
    groups = [  # (count, request, need)
        (3, (0, 0, 0, 0), 0),                                       # the zero request: every node without a negative
        (1, (top, m1 + 1, 8, m3 + 1), 0),                           # a walkable node's whole residual: score 0
        (2, (1000, synth.GiB | LO1, 0, 0), 0),                      # lo20(q1) all ones: every node but ...FFFFF borrows
        (2, (1000, synth.GiB, 0, 10 * synth.GiB | LO3), 0),         # lo24(q3) all ones
        (1, (500, 3 * synth.GiB | 0x80000, 1, synth.GiB | 0x800000), 1),
        (1, (SMAX + 1, 0, 0, 0), 0),                                # walk false: overlay only
        (1, (0, 0, 1 << 20, 0), 0),                                 # walk false: overlay only
        (1, (top - 1, m1, 8, m3), 0),                               # s(q) = SMAX - 2: KQ2 = SMAX << 24
        (1, (top, m1, 8, m3), 0),                                   # s(q) = SMAX - 1: KQ2 saturates
        (1, (SMAX - 2, 0, 0, 0), 0),                                # the same two sums in one term: slow nodes only
        (1, (SMAX - 1, 0, 0, 0), 0),
        (1, (0, (SMAX - 2) << 20 | 3, 0, 0), 0),
        (1, (0, 0, 0, INT64_MAX), 0),
        (4, (1 << 62, synth.GiB, 0, 0), isl),                       # island: count x request saturates at INT64_MAX
        (2, (4000, 8 * synth.GiB | 5, 2, 0), isl | 1),              # island: 2 x request, no saturation
        (1, (INT64_MAX,) * 4, 0),                                   # fits the all-INT64_MAX node, once
        (1, (2000, 4 * synth.GiB | 0x12345, 0, synth.GiB | 0x654321), 0),
        (1, (16_000, 64 * synth.GiB | 0xFFFFE, 8, 100 * synth.GiB | 2), 1),
    ]
    G = len(groups)
    need = np.array([g[2] for g in groups], dtype=np.uint32)
    if variant:
        need[-2:] |= UNKNOWN_LABEL
    return synth.JobBatch(np.arange(G + 1, dtype=np.int32), (np.arange(G, dtype=np.int32) * 37) % 11,
                          np.array([g[0] for g in groups], dtype=np.int32),
                          np.array([g[1] for g in groups], dtype=np.int64), need, np.zeros(G, dtype=np.int8))


def edge_script(cfg):
    """script() for the EDGE_KINDS: the same steps; requests and the update's donor nodes carry low bits."""
    s = 100 * cfg.topk + cfg.n
    slots, op, cap, used, labels, island = make_deltas(cfg.n, 40, s + 5)
    rng = np.random.default_rng(s + 6)
    cap[:, 1] += rng.integers(0, 1 << 20, len(slots)) | 1
    cap[:, 3] += rng.integers(0, 1 << 24, len(slots)) | 1
    if cfg.kind == "thresholds":
        places = [threshold_batch(), threshold_batch(), threshold_batch(), threshold_batch(1)]
    else:
        nz = cfg.kind == "rare_borrow"
        places = [low_bits(batch(6, s + 1), s + 11, nz), low_bits(batch(5, s + 2), s + 12, nz),
                  low_bits(batch(6, s + 3), s + 13, nz), low_bits(batch_d(s + 4), s + 14, nz)]
    return [Step("load", make_inventory(cfg.n, cfg.kind)), Step("place", places[0]), Step("place", places[1]),
            Step("update", (slots, op, cap, used, labels, island)), Step("place", places[2]), Step("place", places[3]),
            Step("reset", None), Step("place", places[0])]


def script(cfg):
    if cfg.kind in EDGE_KINDS:
        return edge_script(cfg)
    s = 100 * cfg.topk + cfg.n
    deltas = make_deltas(cfg.n, 40, s + 5)      # (one node: 40 entries for the same slot, the last one wins)
    return [Step("load", make_inventory(cfg.n, cfg.kind)), Step("place", batch(6, s + 1)), Step("place", batch(5, s + 2)),
            Step("update", deltas), Step("place", batch(6, s + 3)), Step("place", batch_d(s + 4)), Step("reset", None),
            Step("place", batch(6, s + 1))]


def scan_bound(keys):
    """merge_kernel's G for one group's keys by local node (NO_KEY = does not fit), restated from scan_kernel."""
    k = np.asarray(keys, dtype=np.uint64)
    pad = np.full(-(-len(k) // 1024) * 1024, NO_KEY, dtype=np.uint64)
    pad[:len(k)] = k
    lanes = np.sort(pad.reshape(-1, 16, 64), axis=1)     # [wave][node of the lane][lane]
    return int(lanes[:, 1, :].min())                     # the smallest second-best key of any lane


def expected_lists(res, labels, b, groups, K, scan):
    """[(n, limit, keys)] for the window's groups on the residuals `res` ([4][N]) and labels."""
    req = synth.scan_requests(b)
    out = []
    for g in groups:
        k = scan_emulator.keys(res, labels, req[g], int(b.group_need[g]), 0)
        bound = scan_bound(k) if scan else NO_KEY
        B = sorted(int(x) for x in k[k != scan_emulator.NO_KEY] if int(x) < bound)
        out.append((min(K, len(B)), B[K] if len(B) > K else bound, B[:K]))
    return out


def first_window(b):
    """The groups of the batch's first window (the host resolver's own choice)."""
    from placement import Resolver
    return Resolver(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need).next_window(WINDOW_GROUPS,
                                                                                                     WINDOW_PODS)


def read_dump(path):
    """A PE_DUMP_WINDOWS file holding one window -> (list stride, groups, [(n, flags, limit, keys)], seeds)."""
    raw = open(path, "rb").read()
    J, G, stride = struct.unpack_from("<3q", raw, 0)
    at = 24 + 4 * (J + 1) + 4 * J + 4 * G + 32 * G + 4 * G
    (n_total,) = struct.unpack_from("<q", raw, at)
    at += 8 + NODE_STATE_BYTES * n_total
    (wg,) = struct.unpack_from("<i", raw, at)
    groups = list(struct.unpack_from("<%di" % wg, raw, at + 4))
    at += 4 + 4 * wg
    gb = 16 + 8 * stride
    lists = []
    for g in range(wg):
        n, flags, limit = struct.unpack_from("<iiQ", raw, at + g * gb)
        assert 0 <= n <= stride, (n, stride)
        lists.append((n, flags, limit, list(struct.unpack_from("<%dQ" % n, raw, at + g * gb + 16))))
    at += wg * gb
    (ns,) = struct.unpack_from("<i", raw, at)
    assert ns == 0 and at + 4 == len(raw), "one window without seeds expected (%d seeds, %d of %d bytes)" % (ns, at + 4, len(raw))
    return stride, groups, lists, ns


Counts = namedtuple("Counts", "lists full short empty overlay")


def saturating(res):
    """Nodes whose score terms can saturate (pe_node_key.h): the walk evaluates them in its overlay, always."""
    smax = (1 << 40) - 1
    r = np.asarray(res, dtype=np.int64)
    return (r.min(axis=0) >= 0) & ((r[0] > smax) | ((r[1] >> 20) > smax) | (r[2] >= (1 << 20)) | ((r[3] >> 24) > smax))


def node_class(res):
    """node_prep (pe_kernels.hip) restated: per node 0 = never fits (a negative residual, K = 0), 1 = walkable
    (K = S << 24 | gid), 2 = slow (KEY_SLOW: the full formula, the walk's overlay); and S(n) (0 where not walkable)."""
    r = [[int(v) for v in row] for row in np.asarray(res, dtype=np.int64)]
    cls, S = [], []
    for r0, r1, r2, r3 in zip(*r):
        s = r0 + (r1 >> 20) + (r2 << 20) + (r3 >> 24)
        if min(r0, r1, r2, r3) < 0:
            c = 0
        elif r0 > SMAX or r1 >= 1 << 60 or r2 >= 1 << 20:
            c = 2
        else:
            c = 1 if s < SMAX else 2
        cls.append(c)
        S.append(s if c == 1 else 0)
    return np.array(cls, dtype=np.int8), np.array(S, dtype=np.uint64)


def slow_nodes(res):
    return node_class(res)[0] == 2


def model_counts(cfg, scan, slow_of=None):
    """The script on the host model alone: the lists of the calls' first windows; those with K keys and a real limit;
    the short ones whose limit is the bound (the walk: NO_KEY); the empty ones; and those of calls that begin with a
    saturating node in the inventory.  pe_place_greedy rebuilds the walk index when it begins, so at a call's first
    window the overlay holds exactly the saturating nodes: only those calls' lists are taken with a non-empty overlay,
    and every call's first window follows a rebuild.  (slow_of: the test for such nodes; the EDGE_KINDS sit on
    node_prep's own lines and take node_class.)"""
    m, c = None, dict.fromkeys(Counts._fields, 0)
    for st in script(cfg):
        if st.op == "load":
            m = Model.of(st.arg)
        elif st.op == "update":
            m.update(st.arg)
        elif st.op == "reset":
            m.reset()
        else:
            groups = first_window(st.arg)
            assert len(groups) > 0
            slow = bool((slow_of or saturating)(m.res).any())
            for n, limit, _ in expected_lists(m.res, m.labels, st.arg, groups, cfg.topk, scan):
                c["lists"] += 1
                c["full"] += n == cfg.topk and limit != NO_KEY
                c["short"] += 0 < n < cfg.topk and (scan or limit == NO_KEY)
                c["empty"] += n == 0
                c["overlay"] += slow
            m.place(st.arg)
    return Counts(**{k: int(v) for k, v in c.items()})


_totals = {}


def totals(scan):
    """model_counts summed over CONFIGS."""
    if scan not in _totals:
        per = [model_counts(cfg, scan) for cfg in CONFIGS]
        _totals[scan] = Counts(*[sum(x) for x in zip(*per)])
    return _totals[scan]


def edge_totals(scan):
    """model_counts summed over EDGE_CONFIGS."""
    if ("edge", scan) not in _totals:
        per = [model_counts(cfg, scan, slow_nodes) for cfg in EDGE_CONFIGS]
        _totals["edge", scan] = Counts(*[sum(x) for x in zip(*per)])
    return _totals["edge", scan]


def emulated_walk(res, labels, q, need, K, slack=2, multi=2, multi_after=1):
    """walk_kernel restated for one group on the residuals res: rounds of 1024 nodes by K(n), the start rule (the last
    round that begins below s(q) << 24), the per-round can-it-fit test, steps of one round and then up to `multi`, the
    stop test X = rmin(next round) - ((s(q) + slack) << 24) once K + 1 collected keys lie below it, the slow nodes in
    full afterwards (keys below the stop bound only).  slack = 2, the largest borrow count, is the kernel; a smaller
    one is the walk that trusts K(n) order.  The in-walk compaction keeps the K + 1 smallest and changes no answer:
    it is left out.  -> ((n, limit, keys), rounds walked)"""
    res = np.asarray(res, dtype=np.int64)
    q = [int(v) for v in q]
    cls, S = node_class(res)
    k_all = scan_emulator.keys(res, labels, q, need, 0)
    walkable = np.nonzero(cls == 1)[0]
    kn = (S[walkable] << np.uint64(24)) | walkable.astype(np.uint64)
    by_kn = np.argsort(kn, kind="stable")
    order, kn = walkable[by_kn], kn[by_kn]
    nr = -(-len(order) // 1024)
    sq = q[0] + (q[1] >> 20) + (q[3] >> 24)
    sq = SMAX if q[0] > SMAX or q[2] >= 1 << 20 or sq >= SMAX else sq
    sq = sq + (q[2] << 20) if sq < SMAX else sq
    walk = sq < SMAX
    got, xstop, rounds = [], NO_KEY, 0
    if walk and nr:
        rmin = [int(kn[r * 1024]) for r in range(nr)]
        member = [order[r * 1024:(r + 1) * 1024] for r in range(nr)]
        can = [bool((res[:, m].max(axis=1) >= np.array(q)).all()) and
               int(np.bitwise_or.reduce(labels[m])) & need == need for m in member]

        def next_round(r):
            while r < nr and not can[r]:
                r += 1
            return r

        r = next_round(max(sum(x < sq << 24 for x in rmin) - 1, 0))
        while r < nr:
            have = np.concatenate(got) if got else np.zeros(0, np.uint64)
            if len(have) >= K + 1:
                X = 0 if sq + slack >= 1 << 40 else max(rmin[r] - ((sq + slack) << 24), 0)
                if int((have < np.uint64(X)).sum()) >= K + 1:
                    xstop = X
                    break
            step = [r]
            while rounds >= multi_after and len(step) < multi and next_round(step[-1] + 1) < nr:
                step.append(next_round(step[-1] + 1))
            for x in step:
                k = k_all[member[x]]
                got.append(k[k != scan_emulator.NO_KEY])
            r = next_round(step[-1] + 1)
            rounds += len(step)
    slow = k_all[cls == 2]
    got.append(slow[slow < np.uint64(xstop)])
    srt = sorted(int(x) for x in np.concatenate(got))
    return (min(K, len(srt)), srt[K] if len(srt) > K else NO_KEY, srt[:K]), rounds


def walk_constants(path):
    """WK_ROUND, MG_CAP, WK_MULTI and WK_MULTI_AFTER of pe_kernels.h."""
    text = open(path).read()
    out = {}
    for name in ("WK_ROUND", "MG_CAP"):
        out[name] = int(re.search(r"\b%s\s*=\s*(\d+)\s*;" % name, text).group(1))
    for name in ("WK_MULTI", "WK_MULTI_AFTER"):
        out[name] = int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    return out


def first_window_states(cfg):
    """The script on the host model alone: [(residuals, labels, batch, groups of the first window)] per place call."""
    m, out = None, []
    for st in script(cfg):
        if st.op == "load":
            m = Model.of(st.arg)
        elif st.op == "update":
            m.update(st.arg)
        elif st.op == "reset":
            m.reset()
        else:
            out.append((m.res.copy(), m.labels.copy(), st.arg, first_window(st.arg)))
            m.place(st.arg)
    return out
