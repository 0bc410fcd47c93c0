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
residuals: in no list)."""
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

Step = namedtuple("Step", "op arg")


def make_inventory(n, kind, seed=3):
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


def script(cfg):
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


def model_counts(cfg, scan):
    """The script on the host model alone: the lists of the calls' first windows; those with K keys and a real limit;
    the short ones whose limit is the bound (the walk: NO_KEY); the empty ones; and those of calls that begin with a
    saturating node in the inventory.  pe_place_greedy rebuilds the walk index when it begins, so at a call's first
    window the overlay holds exactly the saturating nodes: only those calls' lists are taken with a non-empty overlay,
    and every call's first window follows a rebuild."""
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
            slow = bool(saturating(m.res).any())
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
