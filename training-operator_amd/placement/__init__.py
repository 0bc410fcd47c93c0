"""MI355X gang-placement engine -- Python handle over the libplacement C ABI.

    eng = Engine(device_id=0)                      # one context per process / GPU / shard
    eng.load_nodes(cap, used, labels, island)      # [4][N] int64 SoA of the global inventory
    res, present, members, ovf = eng.pg_min_resources(V1, *csr)   # CalcPGMinResources batch
    counts = eng.fit_mask(req, need)               # J x N feasibility bitmask (device-resident)
    pod_node, status = eng.place_greedy(batch)     # greedy best-fit all-or-nothing gangs

Every call runs on the GPU through include/placement.h; nothing here computes a result itself.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _abi
from ._abi import (PE_CAP_MAX, PE_MAX_DOMAINS, PE_MAX_LEVELS, PE_MAX_PAIR_VICTIMS, PE_MAX_SCALE_NODES, PE_MAX_SPLIT_PARTS, PE_SPLIT_TOO_MANY, PE_SLICE_NODE, PE_JOB_PLACED, PE_JOB_UNSCHEDULABLE, PE_KIND_CONTAINER, PE_KIND_INIT, PE_KIND_OVERHEAD,
                   PE_KIND_SHIFT, PE_KIND_SIDECAR, PE_MODE_V1, PE_MODE_V2, PE_NODE_REMOVE, PE_NODE_SET)

V1, V2 = PE_MODE_V1, PE_MODE_V2

__all__ = ["Engine", "HostExchange", "Resolver", "PlacementError", "V1", "V2", "PE_JOB_PLACED", "PE_JOB_UNSCHEDULABLE",
           "PE_KIND_CONTAINER", "PE_KIND_INIT", "PE_KIND_SIDECAR", "PE_KIND_OVERHEAD", "PE_KIND_SHIFT", "comm_id",
           "PE_NODE_SET", "PE_NODE_REMOVE", "PE_CAP_MAX", "wide_ints", "wide_limbs", "PE_MAX_DOMAINS", "DomainCapacity",
           "select_domain", "PE_MAX_LEVELS", "TreeCapacity", "select_tree", "GangFit", "DrainFit", "ScaleUp", "PE_MAX_SCALE_NODES", "GangPreempt", "PE_MAX_PAIR_VICTIMS",
           "TreeSplit", "split_tree", "PE_MAX_SPLIT_PARTS", "PE_SPLIT_TOO_MANY", "TreeSlices", "PE_SLICE_NODE",
           "FitExplain", "explain_message", "PE_EXPLAIN_BINS", "PE_EXPLAIN_LABELS", "PE_EXPLAIN_ANY"]


class PlacementError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_abi.ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dt) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dt)


def wide_ints(lo, hi) -> np.ndarray:
    """The signed 128-bit values hi * 2^64 + lo of pg_min_resources_wide's (lo u64, hi i64) limb arrays
    as Python ints (an object array of the same shape)."""
    lo = np.asarray(lo, dtype=np.uint64)
    hi = np.asarray(hi, dtype=np.int64)
    out = np.empty(lo.shape, dtype=object)
    flat = out.reshape(-1)
    for i, (a, b) in enumerate(zip(lo.reshape(-1).tolist(), hi.reshape(-1).tolist())):
        flat[i] = (b << 64) + a
    return out


def wide_limbs(values):
    """Non-negative Python ints below 2^128 (any nesting / object array) -> (lo, hi) uint64 limb arrays,
    the request form of pg_min_resources_wide's cont_req_lo / cont_req_hi (the engine takes values
    below 2^127)."""
    v = np.asarray(values, dtype=object)
    lo = np.zeros(v.shape, dtype=np.uint64)
    hi = np.zeros(v.shape, dtype=np.uint64)
    fl, fh = lo.reshape(-1), hi.reshape(-1)
    for i, x in enumerate(v.reshape(-1).tolist()):
        x = int(x)
        if not 0 <= x < 1 << 128:
            raise ValueError(f"{x} has no two-limb form")
        fl[i] = x & (2**64 - 1)
        fh[i] = x >> 64
    return lo, hi


PE_EXPLAIN_BINS = 32
PE_EXPLAIN_LABELS = 4   # signature bit of the label test
PE_EXPLAIN_ANY = -1
EXPLAIN_NAMES = ("cpu", "memory", "amd.com/gpu", "ephemeral-storage")


def explain_message(hist_row, names=EXPLAIN_NAMES) -> str:
    """One job's histogram ([32], ints) in kube-scheduler's manner: "{fits}/{live} nodes are available: {c}
    Insufficient {name}, ..., {c} node(s) didn't match the required labels."  Reasons in the order cpu, memory,
    gpu, ephemeral, labels with INCLUSIVE counts; zero counts are left out; with no reason the text ends after
    "available."."""
    h = [int(v) for v in hist_row]
    incl = [sum(h[s] for s in range(PE_EXPLAIN_BINS) if s >> r & 1) for r in range(5)]
    parts = [f"{incl[d]} Insufficient {names[d]}" for d in range(4) if incl[d]]
    if incl[PE_EXPLAIN_LABELS]:
        parts.append(f"{incl[PE_EXPLAIN_LABELS]} node(s) didn't match the required labels")
    head = f"{h[0]}/{sum(h)} nodes are available"
    return head + (": " + ", ".join(parts) + "." if parts else ".")


class FitExplain(NamedTuple):
    """Engine.fit_explain's answer.  hist int64 [J][32]: live nodes in scope per signature; near uint64 [J][4] or
    None: the smallest shortfall among the nodes failing on dimension d alone, 0 = no such node."""
    hist: np.ndarray
    near: Optional[np.ndarray]

    @property
    def fits(self) -> np.ndarray:             # [J]: pe_fit_mask's count
        return self.hist[:, 0]

    @property
    def live(self) -> np.ndarray:             # [J]: live nodes in scope
        return self.hist.sum(axis=1)

    @property
    def insufficient(self) -> np.ndarray:     # [J][4]: nodes lacking dimension d, alone or not
        bits = np.arange(PE_EXPLAIN_BINS)
        return np.stack([self.hist[:, (bits >> d & 1) == 1].sum(axis=1) for d in range(4)], axis=1)

    @property
    def label_mismatch(self) -> np.ndarray:   # [J]
        return self.hist[:, PE_EXPLAIN_BINS // 2:].sum(axis=1)

    @property
    def only(self) -> np.ndarray:             # [J][4]: nodes failing on dimension d alone
        return self.hist[:, [1, 2, 4, 8]]

    def message(self, j, names=EXPLAIN_NAMES) -> str:
        return explain_message(self.hist[j], names)


class DomainCapacity(NamedTuple):
    """Engine.gang_capacity_domains' answer; a part that was not asked for is None."""
    dom_slots: Optional[np.ndarray]      # int64 [J][n_domains]: pods of job j's shape that domain k holds
    dom_nodes: Optional[np.ndarray]      # int64 [J][n_domains]: its nodes holding at least one
    domain: Optional[np.ndarray]         # int32 [J]: smallest dom_slots >= count, ties to the smallest id; -1 = none
    domain_slots: Optional[np.ndarray]   # int64 [J]: that domain's slots, 0 when none
    feasible: Optional[np.ndarray]       # int32 [J]: domains with dom_slots >= count


def select_domain(dom_slots, count):
    """The selection rule of pe_gang_capacity_domains on a host table: for the shards' dom_slots tables
    ADDED UP ([J][n_domains]; a domain may span shards, so one shard's table must not be selected from)
    and count [J] >= 1, (domain int32[J], domain_slots int64[J], feasible int32[J]) -- the domain with
    the smallest dom_slots >= count, ties to the smallest id, -1 / 0 when none, and how many domains
    hold the gang."""
    t = np.asarray(dom_slots, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.int64).reshape(-1)
    if t.ndim != 2 or cnt.shape != (t.shape[0],):
        raise ValueError("dom_slots must be [J][n_domains] and count [J]")
    if (cnt < 1).any():
        raise ValueError("count must be >= 1")
    ok = t >= cnt[:, None]
    feasible = ok.sum(axis=1).astype(np.int32)
    masked = np.where(ok, t, np.iinfo(np.int64).max)
    domain = np.where(feasible > 0, masked.argmin(axis=1) if t.shape[1] else 0, -1).astype(np.int32)   # argmin: first of equals
    slots = np.where(feasible > 0, masked.min(axis=1) if t.shape[1] else 0, 0).astype(np.int64)
    return domain, slots, feasible


class TreeCapacity(NamedTuple):
    """Engine.gang_capacity_tree's answer; a part that was not asked for is None.  T = sum(level_size); the
    column of domain k of level l is sum(level_size[:l]) + k."""
    tree_slots: Optional[np.ndarray]     # int64 [J][T]: pods of job j's shape that each domain of each level holds
    tree_nodes: Optional[np.ndarray]     # int64 [J][T]: its nodes holding at least one
    level: Optional[np.ndarray]          # int32 [J]: lowest level <= max_level with a domain of slots >= count; -1 = none
    domain: Optional[np.ndarray]         # int32 [J]: that level's domain with the smallest such slots, ties to the smallest id
    domain_slots: Optional[np.ndarray]   # int64 [J]: that domain's slots, 0 when none
    feasible: Optional[np.ndarray]       # int32 [J][n_levels]: domains of each level with slots >= count


class TreeSplit(NamedTuple):
    """Engine.gang_split_tree's and split_tree's answer."""
    level: np.ndarray                    # int32 [J]: gang_capacity_tree's level, -1 = none
    domain: np.ndarray                   # int32 [J]: gang_capacity_tree's domain, -1 = none
    parts: np.ndarray                    # int32 [J]: number of (leaf, pods) parts; 0 = none selected, PE_SPLIT_TOO_MANY
    part_domain: np.ndarray              # int32 [J][max_parts]: the parts' leaf ids in list order, the tail -1
    part_pods: np.ndarray                # int32 [J][max_parts]: their pods (>= 1, adding up to count), the tail 0
    spread: np.ndarray                   # int32 [J][n_levels]: domains of each level the gang touches, 0 above the level


class TreeSlices(NamedTuple):
    """Engine.gang_slice_tree's answer: TreeSplit's, with the selected domain's units."""
    level: np.ndarray                    # int32 [J]: lowest level in [max(slice_level, 0), max_level] with a domain of units >= count / slice_size; -1 = none
    domain: np.ndarray                   # int32 [J]: that level's domain with the smallest such units, ties to the smallest id
    domain_units: np.ndarray             # int64 [J]: that domain's units (whole slices), 0 when none
    parts: np.ndarray                    # int32 [J]: number of (leaf, pods) parts; 0 = none selected, PE_SPLIT_TOO_MANY
    part_domain: np.ndarray              # int32 [J][max_parts]: the parts' leaf ids in list order, the tail -1
    part_pods: np.ndarray                # int32 [J][max_parts]: their pods (>= 1, adding up to count), the tail 0
    spread: np.ndarray                   # int32 [J][n_levels]: domains of each level the gang touches, 0 above the level


class GangFit(NamedTuple):
    """Engine.gang_fit_domains' answer; a part that was not asked for is None."""
    fits: Optional[np.ndarray]           # uint8 [P]: 1 = the job alone would be placed in the domain right now
    fail_group: Optional[np.ndarray]     # int32 [P]: -1, or the first group (within the job) not placed in full
    pods: Optional[np.ndarray]           # int64 [P]: pods the rule had placed when it stopped
    first: Optional[np.ndarray]          # int32 [J]: the smallest fitting pair of job j, -1 = none


class DrainFit(NamedTuple):
    """Engine.drain_fit_domains' answer; a part that was not asked for is None."""
    fits: Optional[np.ndarray]           # uint8 [C]: 1 = the node's pods all find a node in the target domain right now
    moved: Optional[np.ndarray]          # int64 [C]: pods that had found a node when the rule stopped
    fail_slot: Optional[np.ndarray]      # int64 [C]: -1, or the pod slot of the first pod that found no node
    target: Optional[np.ndarray]         # int32 [S]: the node the pod of slot s moves to, -1 = it does not move

    def move_of(self, pod_node, node):
        """(release_pod_node, assume_pod_node) int32 [S] for carrying out the move of candidate node `node`: with the
        book's own gang_group_off, group_count and group_req, release_gangs(..., release_pod_node) gives back what the
        node's pods hold and assume_gangs(..., assume_pod_node) takes it at their targets; every other slot is -1."""
        if self.target is None:
            raise ValueError("the call was made without targets")
        pod = np.asarray(pod_node, dtype=np.int32).reshape(-1)
        if pod.shape != self.target.shape:
            raise ValueError("pod_node must be the call's [S]")
        mine = pod == int(node)
        none = np.int32(-1)
        return np.where(mine, pod, none).astype(np.int32), np.where(mine, self.target, none).astype(np.int32)


class ScaleUp(NamedTuple):
    """Engine.scale_up_domains' answer; a part that was not asked for is None."""
    nodes: Optional[np.ndarray]          # int32 [P]: the fewest new nodes with which the job is placed, -1 = none up to pair_max
    fail_group: Optional[np.ndarray]     # int32 [P]: the deciding attempt's first group not placed in full, -1 = placed
    pods: Optional[np.ndarray]           # int64 [P]: pods the deciding attempt had placed when it stopped
    new_pods: Optional[np.ndarray]       # int64 [P]: those of them that sit on new nodes
    best: Optional[np.ndarray]           # int32 [J]: the pair of job j with the fewest new nodes, ties to the smallest p; -1 = none


class GangPreempt(NamedTuple):
    """Engine.gang_preempt_domains' answer; a part that was not asked for is None."""
    prefix: Optional[np.ndarray]         # int32 [P]: the smallest prefix of the pair's list whose release places the job, -1 = none
    victims: Optional[np.ndarray]        # uint64 [P]: the final set after the fill-back, bit i = position i of the list
    count: Optional[np.ndarray]          # int32 [P]: its popcount, -1 when the prefix is -1
    best: Optional[np.ndarray]           # int32 [J]: the pair of job j with the smallest count >= 0, ties to the smallest p; -1 = none


def _level_sizes(level_size):
    ls = np.asarray(level_size, dtype=np.int64).reshape(-1)
    if not 1 <= len(ls) <= PE_MAX_LEVELS or (ls < 1).any() or (ls > PE_MAX_DOMAINS).any():
        raise ValueError("level_size must hold 1 .. PE_MAX_LEVELS sizes in [1, PE_MAX_DOMAINS]")
    return ls


def select_tree(tree_slots, count, level_size, max_level=None):
    """The selection rule of pe_gang_capacity_tree on a host table: for the shards' tree_slots tables ADDED
    UP ([J][T]; one shard's table must not be selected from), count [J] >= 1 and max_level [J] in
    [0, n_levels) (None = the top level), (level int32[J], domain int32[J], domain_slots int64[J], feasible
    int32[J][n_levels]) -- the lowest level <= max_level at which a domain holds the gang, there the domain
    with the smallest slots >= count (ties to the smallest id), -1 / -1 / 0 when none, and per level how
    many domains hold the gang."""
    ls = _level_sizes(level_size)
    L = len(ls)
    t = np.asarray(tree_slots, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.int64).reshape(-1)
    J = cnt.shape[0]
    if t.ndim != 2 or t.shape != (J, int(ls.sum())):
        raise ValueError("tree_slots must be [J][sum(level_size)] and count [J]")
    ml = np.full(J, L - 1, dtype=np.int64) if max_level is None else np.asarray(max_level, dtype=np.int64).reshape(-1)
    if ml.shape != (J,):
        raise ValueError("max_level must be [J]")
    if (cnt < 1).any():
        raise ValueError("count must be >= 1")
    if ((ml < 0) | (ml >= L)).any():
        raise ValueError("max_level must be in [0, n_levels)")
    level = np.full(J, -1, dtype=np.int32)
    domain = np.full(J, -1, dtype=np.int32)
    slots = np.zeros(J, dtype=np.int64)
    feasible = np.zeros((J, L), dtype=np.int32)
    off = 0
    for l in range(L):
        d, s, f = select_domain(t[:, off:off + int(ls[l])], cnt)
        feasible[:, l] = f
        take = (level < 0) & (ml >= l) & (f > 0)
        level[take], domain[take], slots[take] = l, d[take], s[take]
        off += int(ls[l])
    return level, domain, slots, feasible


def _split_children(a, ids, slots):
    """One parent's step of pe_gang_split_tree: allotment a over the children (ids ascending, their slots) ->
    [(child, pods)], the whole parts in walk order, then the last part."""
    order = sorted(range(len(ids)), key=lambda i: (-slots[i], ids[i]))
    out, r = [], a
    for pos, i in enumerate(order):
        if slots[i] >= r:
            last = min((x for x in order[pos:] if slots[x] >= r), key=lambda x: (slots[x], ids[x]))
            return out + [(ids[last], r)]
        out.append((ids[i], slots[i]))
        r -= slots[i]
    raise ValueError("tree_slots is not the roll-up of its children along parent")


def split_tree(tree_slots, count, level_size, parent=None, max_level=None, max_parts=PE_MAX_SPLIT_PARTS) -> TreeSplit:
    """The rule of pe_gang_split_tree on a host table: for the shards' tree_slots tables ADDED UP ([J][T]),
    count [J] >= 1, the hierarchy (level_size, parent) the tables were made with and max_level [J] or None, the
    selection of select_tree followed by the descent that spreads each gang over the fewest domains of every
    level below.  max_parts in [1, PE_MAX_SPLIT_PARTS]; a job whose list passes it at any level has parts =
    PE_SPLIT_TOO_MANY, rows -1 / 0 and spread 0."""
    ls = _level_sizes(level_size)
    L = len(ls)
    if not 1 <= int(max_parts) <= PE_MAX_SPLIT_PARTS:
        raise ValueError("max_parts must be in [1, PE_MAX_SPLIT_PARTS]")
    mp = int(max_parts)
    level, domain, _, _ = select_tree(tree_slots, count, ls, max_level)
    t = np.asarray(tree_slots, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.int64).reshape(-1)
    J = cnt.shape[0]
    off = np.concatenate([[0], np.cumsum(ls)]).astype(np.int64)
    par = np.zeros(0, dtype=np.int64) if parent is None else np.asarray(parent, dtype=np.int64).reshape(-1)
    if len(par) != int(off[L] - ls[-1]):
        raise ValueError("parent must be [sum(level_size) - level_size[-1]]")
    kids = [None] + [[np.flatnonzero(par[off[l - 1]:off[l]] == p) for p in range(int(ls[l]))] for l in range(1, L)]
    parts = np.zeros(J, dtype=np.int32)
    part_domain = np.full((J, mp), -1, dtype=np.int32)
    part_pods = np.zeros((J, mp), dtype=np.int32)
    spread = np.zeros((J, L), dtype=np.int32)
    for j in range(J):
        if level[j] < 0:
            continue
        cur = [(int(domain[j]), int(cnt[j]))]
        sp = [0] * L
        sp[level[j]] = 1
        for l in range(int(level[j]), 0, -1):
            nxt = []
            for p, a in cur:
                ids = kids[l][p]
                nxt += _split_children(a, ids.tolist(), t[j, off[l - 1] + ids].tolist())
                if len(nxt) > mp:
                    break
            cur = nxt
            sp[l - 1] = len(cur)
            if len(cur) > mp:
                break
        if len(cur) > mp:
            parts[j] = PE_SPLIT_TOO_MANY
            continue
        parts[j] = len(cur)
        spread[j] = sp
        part_domain[j, :len(cur)] = [c for c, _ in cur]
        part_pods[j, :len(cur)] = [n for _, n in cur]
    return TreeSplit(level, domain, parts, part_domain, part_pods, spread)


def comm_id() -> bytes:
    buf = (ctypes.c_uint8 * _abi.PE_COMM_ID_BYTES)()
    rc = _abi.load().pe_comm_id(buf)
    if rc != 0:
        raise PlacementError(rc, "pe_comm_id failed")
    return bytes(buf)


class HostExchange:
    """pe_host_exchange: the native shared-memory all-gather of one node's ranks (the sharded greedy's
    transport when RCCL cannot be set up).  Every rank opens the same `name` ("/..."); rank 0 creates
    the segment.  Pass it as Engine(..., exchange=hx): the engine calls the C function directly (no
    Python on the window path)."""

    def __init__(self, name: str, rank: int, world: int, max_bytes: int):
        self.lib = _abi.load()
        h = ctypes.c_void_p()
        rc = self.lib.pe_host_exchange_open(name.encode(), rank, world, max_bytes, ctypes.byref(h))
        if rc != 0:
            raise PlacementError(rc, f"pe_host_exchange_open({name!r}, rank {rank} of {world})")
        self.h = h
        self.rank, self.world = rank, world
        self.fn = ctypes.cast(self.lib.pe_host_exchange_allgather, _abi.ALLGATHER_FN)

    def allgather(self, blob: bytes) -> bytes:
        out = ctypes.create_string_buffer(len(blob) * self.world)
        rc = self.lib.pe_host_exchange_allgather(self.h, blob, out, len(blob))
        if rc != 0:
            raise PlacementError(rc, "pe_host_exchange_allgather")
        return out.raw

    def close(self):
        if getattr(self, "h", None):
            self.lib.pe_host_exchange_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Engine:
    """One pe_ctx: a GPU, a node-inventory shard, a stream."""

    def __init__(self, device_id: int = 0, rank: int = 0, world_size: int = 1, comm: Optional[bytes] = None,
                 exchange=None, max_nodes: int = 0, gpu_resource_name: str = "amd.com/gpu", topk: int = 0,
                 window_groups: int = 0, window_pods: int = 0, fit_path_mask: int = 0, greedy_flags: int = 0,
                 resort_nodes: int = 0):
        self.lib = _abi.load()
        self._keep = []
        cfg = _abi.PeConfig()
        cfg.device_id = device_id
        cfg.rank = rank
        cfg.world_size = world_size
        if comm is not None:
            cbuf = ctypes.create_string_buffer(bytes(comm), _abi.PE_COMM_ID_BYTES)
            self._keep.append(cbuf)
            cfg.comm_id = ctypes.cast(cbuf, ctypes.c_void_p)
        if isinstance(exchange, HostExchange):   # the native transport: C function + handle
            self._keep.append(exchange)
            cfg.exchange = exchange.fn
            cfg.exchange_user = exchange.h
        elif exchange is not None:
            # exchange(send: bytes) -> bytes (all ranks' blocks concatenated)
            def _cb(user, send, recv, nbytes):
                try:
                    out = exchange(ctypes.string_at(send, nbytes))
                    ctypes.memmove(recv, out, len(out))
                    return 0
                except Exception:  # noqa: BLE001 - reported to the C side as a failure code
                    return 1
            fn = _abi.ALLGATHER_FN(_cb)
            self._keep.append(fn)
            cfg.exchange = fn
        cfg.max_nodes = max_nodes
        self._gname = gpu_resource_name.encode()
        cfg.gpu_resource_name = self._gname
        cfg.topk = topk
        cfg.window_groups = window_groups
        cfg.window_pods = window_pods
        cfg.fit_path_mask = fit_path_mask
        cfg.greedy_flags = greedy_flags
        cfg.resort_nodes = resort_nodes
        self._cfg = cfg
        h = ctypes.c_void_p()
        rc = self.lib.pe_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            raise PlacementError(rc, "pe_create failed (no GPU? the engine has no CPU fallback)")
        self.h = h
        self.rank, self.world_size = rank, world_size
        self.n_nodes = 0
        self.mask_ptr = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.pe_destroy(self.h)
            self.h = None
            self.mask_ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _chk(self, rc: int, what: str, ok=(0,)):
        if rc not in ok:
            raise PlacementError(rc, f"{what}: {self.lib.pe_last_error(self.h).decode(errors='replace')}")
        return rc

    # ------------------------------------------------------------ inventory
    def load_nodes(self, cap, used, labels=None, island=None):
        cap = _c(cap, np.int64)
        used = _c(used, np.int64)
        n = cap.shape[1]
        lab = None if labels is None else _c(labels, np.uint32)
        isl = None if island is None else _c(island, np.int32)
        self._chk(self.lib.pe_load_nodes(self.h, n, _p(cap), _p(used), _p(lab), _p(isl)), "pe_load_nodes")
        self.n_nodes = n
        self.mask_ptr = 0

    def update_nodes(self, slots, op, cap=None, used=None, labels=None, island=None):
        """pe_update_nodes: per entry op 0 (NODE_SET: cap[i][4], used[i][4], labels, island replace
        the slot) or 1 (NODE_REMOVE).  cap/used are row-major [n][4]."""
        slots = _c(slots, np.int64)
        op = _c(op, np.uint8)
        n = slots.shape[0]
        cap = None if cap is None else _c(cap, np.int64)
        used = None if used is None else _c(used, np.int64)
        lab = None if labels is None else _c(labels, np.uint32)
        isl = None if island is None else _c(island, np.int32)
        self._chk(self.lib.pe_update_nodes(self.h, n, _p(slots), _p(op), _p(cap), _p(used), _p(lab), _p(isl)),
                  "pe_update_nodes")

    def reset_residuals(self):
        self._chk(self.lib.pe_reset_residuals(self.h), "pe_reset_residuals")

    def shard_range(self):
        b, e = ctypes.c_int64(), ctypes.c_int64()
        self._chk(self.lib.pe_shard_range(self.h, ctypes.byref(b), ctypes.byref(e)), "pe_shard_range")
        return b.value, e.value

    def comm_ranks(self) -> int:
        """ncclCommCount of the context's RCCL communicator (0 = host exchange / none)."""
        v = ctypes.c_int32()
        self._chk(self.lib.pe_comm_ranks(self.h, ctypes.byref(v)), "pe_comm_ranks")
        return v.value

    def read_residuals(self) -> np.ndarray:
        b, e = self.shard_range()
        out = np.zeros((4, e - b), dtype=np.int64)
        self._chk(self.lib.pe_read_residuals(self.h, _p(out)), "pe_read_residuals")
        return out

    # ------------------------------------------------------------ aggregation
    def pg_min_resources(self, mode, job_group_off, min_member, group_replicas, group_cont_off, cont_req,
                         cont_flags, allow_overflow=True):
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        mm = None if min_member is None else _c(min_member, np.int32)
        rep = _c(group_replicas, np.int32)
        gco = _c(group_cont_off, np.int32)
        req = _c(cont_req, np.int64).reshape(-1, 4)
        fl = _c(cont_flags, np.uint8)
        out = np.zeros((J, 4), dtype=np.int64)
        pres = np.zeros(J, dtype=np.uint8)
        mem = np.zeros(J, dtype=np.int32)
        ovf = np.zeros(J, dtype=np.uint8)
        rc = self.lib.pe_pg_min_resources(self.h, mode, J, _p(jgo), _p(mm), _p(rep), _p(gco), _p(req), _p(fl),
                                          _p(out), _p(pres), _p(mem), _p(ovf))
        self._chk(rc, "pe_pg_min_resources", ok=(0, _abi.PE_EOVERFLOW) if allow_overflow else (0,))
        return out, pres, mem, ovf

    def pg_min_resources_keys(self, mode, job_group_off, min_member, group_replicas, group_cont_off, cont_req,
                              cont_flags, allow_overflow=True):
        """pe_pg_min_resources_keys: cont_req [C][n_keys] int64 (each key at the caller's decimal scale),
        cont_flags [C] u32 = presence bits 0..n_keys-1 | kind << PE_KEYS_KIND_SHIFT.  Returns
        (min_res [J][n_keys], present [J] u16, members, overflow)."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        mm = None if min_member is None else _c(min_member, np.int32)
        rep = _c(group_replicas, np.int32)
        gco = _c(group_cont_off, np.int32)
        req = np.ascontiguousarray(cont_req, dtype=np.int64)
        if req.ndim != 2:
            raise ValueError("cont_req must be [C][n_keys]")
        nk = req.shape[1]
        fl = _c(cont_flags, np.uint32)
        out = np.zeros((J, nk), dtype=np.int64)
        pres = np.zeros(J, dtype=np.uint16)
        mem = np.zeros(J, dtype=np.int32)
        ovf = np.zeros(J, dtype=np.uint8)
        rc = self.lib.pe_pg_min_resources_keys(self.h, mode, J, nk, _p(jgo), _p(mm), _p(rep), _p(gco), _p(req), _p(fl),
                                               _p(out), _p(pres), _p(mem), _p(ovf))
        self._chk(rc, "pe_pg_min_resources_keys", ok=(0, _abi.PE_EOVERFLOW) if allow_overflow else (0,))
        return out, pres, mem, ovf

    def pg_min_resources_wide(self, mode, job_group_off, min_member, group_replicas, group_cont_off, cont_req_lo,
                              cont_flags, cont_req_hi=None, allow_overflow=True):
        """pe_pg_min_resources_wide: the key-table aggregation with exact answers past int64.  A request
        is cont_req_hi * 2^64 + cont_req_lo ([C][n_keys]; without cont_req_hi the low limbs are int64
        values, as in pg_min_resources_keys).  Returns (lo [J][n_keys] u64, hi [J][n_keys] i64, present
        [J] u16, members, overflow): the signed 128-bit sums hi:lo (wide_ints), overflow 0 = the int64 path
        answered, 1 = exact 128-bit value, 2 = left 128 bits (values 0; the call's code is PE_EOVERFLOW)."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        mm = None if min_member is None else _c(min_member, np.int32)
        rep = _c(group_replicas, np.int32)
        gco = _c(group_cont_off, np.int32)
        if cont_req_hi is None:
            lo = np.ascontiguousarray(cont_req_lo, dtype=np.int64)
            hi = None
        else:
            lo = np.ascontiguousarray(cont_req_lo, dtype=np.uint64)
            hi = np.ascontiguousarray(cont_req_hi, dtype=np.uint64)
            if hi.shape != lo.shape:
                raise ValueError("cont_req_hi must have cont_req_lo's shape")
        if lo.ndim != 2:
            raise ValueError("cont_req_lo must be [C][n_keys]")
        nk = lo.shape[1]
        fl = _c(cont_flags, np.uint32)
        out_lo = np.zeros((J, nk), dtype=np.uint64)
        out_hi = np.zeros((J, nk), dtype=np.int64)
        pres = np.zeros(J, dtype=np.uint16)
        mem = np.zeros(J, dtype=np.int32)
        ovf = np.zeros(J, dtype=np.uint8)
        rc = self.lib.pe_pg_min_resources_wide(self.h, mode, J, nk, _p(jgo), _p(mm), _p(rep), _p(gco), _p(lo), _p(hi),
                                               _p(fl), _p(out_lo), _p(out_hi), _p(pres), _p(mem), _p(ovf))
        self._chk(rc, "pe_pg_min_resources_wide", ok=(0, _abi.PE_EOVERFLOW) if allow_overflow else (0,))
        return out_lo, out_hi, pres, mem, ovf

    # ------------------------------------------------------------ fit mask
    def jobs_upload(self, req, need=None):
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        self.fit_jobs = req.shape[0]
        self.mask_ptr = 0
        self._chk(self.lib.pe_jobs_upload(self.h, req.shape[0], _p(req), _p(nd)), "pe_jobs_upload")

    def fit_mask_run(self):
        self._chk(self.lib.pe_fit_mask_run(self.h), "pe_fit_mask_run")

    def fit_counts(self) -> np.ndarray:
        out = np.zeros(self.fit_jobs, dtype=np.int64)
        self._chk(self.lib.pe_fit_counts(self.h, _p(out)), "pe_fit_counts")
        return out

    def fit_mask(self, req, need=None) -> np.ndarray:
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        counts = np.zeros(req.shape[0], dtype=np.int64)
        dptr, wpr = ctypes.c_void_p(), ctypes.c_int64()
        self._chk(self.lib.pe_fit_mask(self.h, req.shape[0], _p(req), _p(nd), _p(counts), ctypes.byref(dptr),
                                       ctypes.byref(wpr)), "pe_fit_mask")
        self.fit_jobs = req.shape[0]
        self.words_per_row = wpr.value
        self.mask_ptr = int(dptr.value or 0)   # valid until the next fit_mask, jobs_upload, load_nodes or close
        return counts

    def mask_extent(self) -> int:
        """u64 words of the device mask that the current layout's formula addresses (include/placement.h)."""
        b, e = self.shard_range()
        J, S, layout = self.fit_jobs, e - b, self.fit_mask_layout()
        Wn = (S + 63) // 64
        if layout == _abi.PE_MASK_NODE_TILES:
            return (J + 15) // 16 * ((Wn + 3) // 4) * 64
        if layout == _abi.PE_MASK_JOB_BITS:
            return (J + 63) // 64 * ((S + 1023) // 1024 * 1024)
        if layout == _abi.PE_MASK_NODE_BLOCKS:
            return (S + 8191) // 8192 * J * 128
        return J * self.fit_mask_row_pitch()

    def read_mask_words(self, n_words: int) -> np.ndarray:
        """The first n_words u64 words at the device pointer the last fit_mask returned: pe_synchronize, then one
        synchronous device-to-host copy.  At most mask_extent() words."""
        if not self.mask_ptr:
            raise PlacementError(_abi.PE_ESTATE, "read_mask_words: no device mask pointer held (fit_mask first)")
        n = int(n_words)
        if not 0 <= n <= self.mask_extent():
            raise PlacementError(_abi.PE_EINVAL, f"read_mask_words: {n} words outside the layout's {self.mask_extent()}")
        self.synchronize()
        out = np.zeros(n, dtype=np.uint64)
        if n:
            rc = _abi.hip_memcpy()(_p(out), ctypes.c_void_p(self.mask_ptr), ctypes.c_size_t(8 * n), _abi.HIP_MEMCPY_D2H)
            if rc != 0:
                raise PlacementError(_abi.PE_EHIP, f"read_mask_words: hipMemcpy returned {rc}")
        return out

    def fit_mask_layout(self) -> int:
        v = ctypes.c_int32()
        self._chk(self.lib.pe_fit_mask_layout(self.h, ctypes.byref(v)), "pe_fit_mask_layout")
        return v.value

    def fit_mask_row_pitch(self) -> int:
        v = ctypes.c_int64()
        self._chk(self.lib.pe_fit_mask_row_pitch(self.h, ctypes.byref(v)), "pe_fit_mask_row_pitch")
        return v.value

    def fit_mask_rows(self, row0: int, n_rows: int) -> np.ndarray:
        b, e = self.shard_range()
        w = (e - b + 63) // 64
        out = np.zeros((n_rows, w), dtype=np.uint64)
        self._chk(self.lib.pe_fit_mask_rows(self.h, row0, n_rows, _p(out)), "pe_fit_mask_rows")
        return out

    # ------------------------------------------------------------ gang capacity
    def gang_capacity(self, req, need=None):
        """pe_gang_capacity: per job shape (req [J][4], need [J] or None) how many pods of that shape this
        shard's current residuals hold.  Returns (slots int64[J], max_node int32[J], nodes int64[J]): the
        sum over the nodes, the largest single node (saturating at PE_CAP_MAX) and the nodes holding at
        least one.  Read-only: residuals and the staged fit batch are untouched."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        slots = np.zeros(J, dtype=np.int64)
        max_node = np.zeros(J, dtype=np.int32)
        nodes = np.zeros(J, dtype=np.int64)
        self._chk(self.lib.pe_gang_capacity(self.h, J, _p(req), _p(nd), _p(slots), _p(max_node), _p(nodes)),
                  "pe_gang_capacity")
        return slots, max_node, nodes

    def fit_explain(self, req, need=None, job_domain=None, level=0, level_size=None, parent=None,
                    near=True) -> "FitExplain":
        """pe_fit_explain: why job j's shape (req [J][4], need [J] or None) fits no node -- per job the shard's
        live nodes counted by 5-bit signature (bit d: req_d > res_d, bit 4: labels) and, with near=True, per
        dimension the smallest shortfall among the nodes that fail on that dimension alone.  job_domain ([J] or
        None = the whole shard; PE_EXPLAIN_ANY = the whole shard for that job) restricts job j to one domain of
        `level` in the hierarchy level_size / parent, exactly as for place_greedy_domains.  Works on a sharded
        context: add the shards' hist and take the minimum of the non-zero near values.  Read-only."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        jd = None if job_domain is None else _c(job_domain, np.int32)
        if jd is not None and jd.shape != (J,):
            raise ValueError("job_domain must be [J]")
        ls = None if level_size is None else _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        if jd is not None and ls is None:
            raise ValueError("job_domain needs level_size")
        hist = np.zeros((J, PE_EXPLAIN_BINS), dtype=np.int64)
        nv = np.zeros((J, 4), dtype=np.uint64) if near else None
        self._chk(self.lib.pe_fit_explain(self.h, J, _p(req), _p(nd), _p(jd), int(level), 0 if ls is None else len(ls),
                                          _p(ls), _p(par), _p(hist), _p(nv)),
                  "pe_fit_explain")
        return FitExplain(hist, nv)

    def gang_capacity_domains(self, req, need=None, count=None, n_domains=None, tables=True) -> DomainCapacity:
        """pe_gang_capacity_domains: gang capacity per topology domain, the domain of a node being its
        island id in [0, n_domains).  With tables=True the [J][n_domains] tables dom_slots / dom_nodes come
        back; with count ([J], >= 1) the device also selects per job the best-fitting domain (domain,
        domain_slots, feasible) -- with tables=False nothing but those J-sized answers crosses.  On a
        sharded context only the tables are available: add them over the shards and use select_domain.
        Read-only, like gang_capacity."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        if n_domains is None:
            raise ValueError("n_domains is required")
        cnt = None if count is None else _c(count, np.int32)
        if cnt is not None and cnt.shape != (J,):
            raise ValueError("count must be [J]")
        D = int(n_domains)
        big = tables and 1 <= D <= PE_MAX_DOMAINS   # (an n_domains the engine refuses allocates nothing here)
        dom_slots = np.zeros((J, D), dtype=np.int64) if big else None
        dom_nodes = np.zeros((J, D), dtype=np.int64) if big else None
        sel = cnt is not None
        domain = np.full(J, -1, dtype=np.int32) if sel else None
        domain_slots = np.zeros(J, dtype=np.int64) if sel else None
        feasible = np.zeros(J, dtype=np.int32) if sel else None
        self._chk(self.lib.pe_gang_capacity_domains(self.h, J, _p(req), _p(nd), _p(cnt), D, _p(dom_slots), _p(dom_nodes),
                                                    _p(domain), _p(domain_slots), _p(feasible)),
                  "pe_gang_capacity_domains")
        return DomainCapacity(dom_slots, dom_nodes, domain, domain_slots, feasible)

    def gang_capacity_tree(self, req, need=None, count=None, max_level=None, level_size=None, parent=None,
                           tables=True) -> TreeCapacity:
        """pe_gang_capacity_tree: gang capacity over a hierarchy of topology levels.  level_size [n_levels]
        (level 0 = the leaf level, the nodes' island ids in [0, level_size[0])); parent [T - level_size[-1]]:
        parent[off_l + k] = the level-(l + 1) domain holding domain k of level l, or -1 (None allowed with one
        level).  With tables=True the [J][T] tables tree_slots / tree_nodes come back; with count ([J], >= 1)
        the device also selects per job the lowest level <= max_level ([J] or None = the top level) at which
        one domain holds the gang and the best-fitting domain there (level, domain, domain_slots, feasible
        [J][n_levels]) -- with tables=False nothing but those answers crosses.  On a sharded context only the
        tables are available: add them over the shards and use select_tree.  Read-only, like gang_capacity."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        L = len(ls)
        cnt = None if count is None else _c(count, np.int32)
        if cnt is not None and cnt.shape != (J,):
            raise ValueError("count must be [J]")
        ml = None if max_level is None else _c(max_level, np.int32)
        if ml is not None and ml.shape != (J,):
            raise ValueError("max_level must be [J]")
        if ml is not None and cnt is None:
            raise ValueError("max_level needs count")
        valid = 1 <= L <= PE_MAX_LEVELS and bool(((ls >= 1) & (ls <= PE_MAX_DOMAINS)).all())
        T = int(ls.astype(np.int64).sum()) if valid else 0
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        if valid and par is not None and len(par) != T - int(ls[-1]):
            raise ValueError("parent must be [sum(level_size) - level_size[-1]]")
        big = tables and valid   # (a hierarchy the engine refuses allocates nothing here)
        tree_slots = np.zeros((J, T), dtype=np.int64) if big else None
        tree_nodes = np.zeros((J, T), dtype=np.int64) if big else None
        sel = cnt is not None
        level = np.full(J, -1, dtype=np.int32) if sel else None
        domain = np.full(J, -1, dtype=np.int32) if sel else None
        domain_slots = np.zeros(J, dtype=np.int64) if sel else None
        feasible = np.zeros((J, max(L, 1)), dtype=np.int32) if sel else None
        self._chk(self.lib.pe_gang_capacity_tree(self.h, J, _p(req), _p(nd), _p(cnt), _p(ml), L, _p(ls), _p(par),
                                                 _p(tree_slots), _p(tree_nodes), _p(level), _p(domain),
                                                 _p(domain_slots), _p(feasible)),
                  "pe_gang_capacity_tree")
        return TreeCapacity(tree_slots, tree_nodes, level, domain, domain_slots, feasible)

    def gang_split_tree(self, req, need=None, count=None, max_level=None, level_size=None, parent=None,
                        max_parts=64) -> TreeSplit:
        """pe_gang_split_tree: gang_capacity_tree's selection (level, domain) followed, on the device, by the
        descent that spreads each gang over the fewest domains of every level below the selected one.  Arguments
        as gang_capacity_tree (count is required); max_parts in [1, PE_MAX_SPLIT_PARTS] is the width of the part
        rows.  parts[j] (leaf, pods) pairs in part_domain[j] / part_pods[j], whose pods add up to count[j] on
        distinct leaves; parts 0 = no level holds the gang, PE_SPLIT_TOO_MANY = more than max_parts domains at
        some level.  On a sharded context add the shards' tree_slots and use split_tree.  Read-only."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        L = len(ls)
        cnt = None if count is None else _c(count, np.int32)
        if cnt is not None and cnt.shape != (J,):
            raise ValueError("count must be [J]")
        ml = None if max_level is None else _c(max_level, np.int32)
        if ml is not None and ml.shape != (J,):
            raise ValueError("max_level must be [J]")
        valid = 1 <= L <= PE_MAX_LEVELS and bool(((ls >= 1) & (ls <= PE_MAX_DOMAINS)).all())
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        if valid and par is not None and len(par) != int(ls.astype(np.int64).sum()) - int(ls[-1]):
            raise ValueError("parent must be [sum(level_size) - level_size[-1]]")
        mp = int(max_parts)
        w = mp if 1 <= mp <= PE_MAX_SPLIT_PARTS else 1   # (a max_parts the engine refuses allocates nothing here)
        level = np.full(J, -1, dtype=np.int32)
        domain = np.full(J, -1, dtype=np.int32)
        parts = np.zeros(J, dtype=np.int32)
        part_domain = np.full((J, w), -1, dtype=np.int32)
        part_pods = np.zeros((J, w), dtype=np.int32)
        spread = np.zeros((J, max(L, 1)), dtype=np.int32)
        self._chk(self.lib.pe_gang_split_tree(self.h, J, _p(req), _p(nd), _p(cnt), _p(ml), L, _p(ls), _p(par), mp,
                                              _p(level), _p(domain), _p(parts), _p(part_domain), _p(part_pods),
                                              _p(spread)),
                  "pe_gang_split_tree")
        return TreeSplit(level, domain, parts, part_domain, part_pods, spread)

    def gang_slice_tree(self, req, need=None, count=None, slice_size=None, slice_level=None, max_level=None,
                        level_size=None, parent=None, max_parts=64) -> TreeSlices:
        """pe_gang_slice_tree: gang_split_tree for gangs made of slices of slice_size[j] pods ([J] or None = 1) that
        must each sit inside one domain of level slice_level[j] ([J] or None = 0; PE_SLICE_NODE = inside one node).
        Capacity counts whole slices at and above the slice level -- a block's units are the sum of its racks'
        units -- and pods below it; count[j] must be a multiple of slice_size[j] and max_level[j] at least
        max(slice_level[j], 0).  With slice_level >= 0 the parts are placed as gang_split_tree's; with PE_SLICE_NODE
        part (leaf, a * z) is one job of a groups {count z, need | PE_NEED_ISLAND} in that leaf.  A sharded context
        refuses the call.  Read-only."""
        req = _c(req, np.int64).reshape(-1, 4)
        nd = None if need is None else _c(need, np.uint32)
        J = req.shape[0]
        if nd is not None and nd.shape != (J,):
            raise ValueError("need must be [J]")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        L = len(ls)
        per_job = {}
        for name, v in (("count", count), ("slice_size", slice_size), ("slice_level", slice_level), ("max_level", max_level)):
            per_job[name] = None if v is None else _c(v, np.int32)
            if per_job[name] is not None and per_job[name].shape != (J,):
                raise ValueError(name + " must be [J]")
        valid = 1 <= L <= PE_MAX_LEVELS and bool(((ls >= 1) & (ls <= PE_MAX_DOMAINS)).all())
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        if valid and par is not None and len(par) != int(ls.astype(np.int64).sum()) - int(ls[-1]):
            raise ValueError("parent must be [sum(level_size) - level_size[-1]]")
        mp = int(max_parts)
        w = mp if 1 <= mp <= PE_MAX_SPLIT_PARTS else 1   # (a max_parts the engine refuses allocates nothing here)
        level = np.full(J, -1, dtype=np.int32)
        domain = np.full(J, -1, dtype=np.int32)
        units = np.zeros(J, dtype=np.int64)
        parts = np.zeros(J, dtype=np.int32)
        part_domain = np.full((J, w), -1, dtype=np.int32)
        part_pods = np.zeros((J, w), dtype=np.int32)
        spread = np.zeros((J, max(L, 1)), dtype=np.int32)
        self._chk(self.lib.pe_gang_slice_tree(self.h, J, _p(req), _p(nd), _p(per_job["count"]), _p(per_job["slice_size"]),
                                              _p(per_job["slice_level"]), _p(per_job["max_level"]), L, _p(ls), _p(par), mp,
                                              _p(level), _p(domain), _p(units), _p(parts), _p(part_domain), _p(part_pods),
                                              _p(spread)),
                  "pe_gang_slice_tree")
        return TreeSlices(level, domain, units, parts, part_domain, part_pods, spread)

    # ------------------------------------------------------------ greedy
    def place_greedy(self, job_group_off, priority, group_count, group_req, group_need=None):
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        P = int(cnt.sum())
        pod = np.full(max(P, 1), -1, dtype=np.int32)
        st = np.zeros(max(J, 1), dtype=np.int32)
        self._chk(self.lib.pe_place_greedy(self.h, J, _p(jgo), _p(_c(priority, np.int32)), _p(cnt), _p(req), _p(nd),
                                           _p(pod), _p(st)), "pe_place_greedy")
        return pod[:P], st[:J]

    def place_batch(self, batch):
        return self.place_greedy(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                 batch.group_need)

    def place_greedy_domains(self, job_group_off, priority, group_count, group_req, group_need, job_domain, level,
                             level_size, parent=None):
        """pe_place_greedy_domains: place_greedy with job j's pods confined to the nodes whose level-`level`
        domain is job_domain[j] ([J], each in [0, level_size[level])).  level_size / parent describe the hierarchy
        exactly as for gang_capacity_tree (parent None allowed with one level); one call has one level.
        Residuals are updated in place.  Returns (pod_node, job_status) like place_greedy."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        dom = None if job_domain is None else _c(job_domain, np.int32)
        if dom is not None and dom.shape != (J,):
            raise ValueError("job_domain must be [J]")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        P = int(np.clip(cnt, 0, None).astype(np.int64).sum())
        pod = np.full(max(P, 1), -1, dtype=np.int32)
        st = np.zeros(max(J, 1), dtype=np.int32)
        self._chk(self.lib.pe_place_greedy_domains(self.h, J, _p(jgo), _p(_c(priority, np.int32)), _p(cnt), _p(req),
                                                   _p(nd), _p(dom), int(level), len(ls), _p(ls), _p(par), _p(pod),
                                                   _p(st)), "pe_place_greedy_domains")
        return pod[:P], st[:J]

    def place_min_member_domains(self, job_group_off, priority, group_count, group_req, group_need, min_member,
                                 job_domain, level, level_size, parent=None):
        """pe_place_min_member_domains: place_greedy_domains for gangs that are schedulable at min_member[j] pods
        ([J]; PE_MIN_MEMBER_ALL = -1 or min_member None: the whole job).  The mandatory pods -- the job's first
        min_member pod slots, plus the rest of an island group the cut falls in -- are placed all-or-nothing; after
        that the optional pods of every group are placed as far as they fit, the rest of the group stays -1.
        Residuals are updated in place.  Returns (pod_node [P], job_status [J], group_pods int32[G], job_pods
        int64[J]): group_pods / job_pods count the pods that hold a node."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        mm = None if min_member is None else _c(min_member, np.int32)
        if mm is not None and mm.shape != (J,):
            raise ValueError("min_member must be [J]")
        dom = None if job_domain is None else _c(job_domain, np.int32)
        if dom is not None and dom.shape != (J,):
            raise ValueError("job_domain must be [J]")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        G = len(cnt)
        P = int(np.clip(cnt, 0, None).astype(np.int64).sum())
        pod = np.full(max(P, 1), -1, dtype=np.int32)
        st = np.zeros(max(J, 1), dtype=np.int32)
        gp = np.zeros(max(G, 1), dtype=np.int32)
        jp = np.zeros(max(J, 1), dtype=np.int64)
        self._chk(self.lib.pe_place_min_member_domains(self.h, J, _p(jgo), _p(_c(priority, np.int32)), _p(cnt), _p(req),
                                                       _p(nd), _p(mm), _p(dom), int(level), len(ls), _p(ls), _p(par),
                                                       _p(pod), _p(st), _p(gp), _p(jp)), "pe_place_min_member_domains")
        return pod[:P], st[:J], gp[:G], jp[:J]

    def gang_fit_domains(self, job_group_off, group_count, group_req, group_need, pair_job, pair_domain, level,
                         level_size, parent=None, tables=True, first=True) -> GangFit:
        """pe_gang_fit_domains: for every pair p, would place_greedy_domains place job pair_job[p] ALONE in the
        level-`level` domain pair_domain[p] against the current residuals?  Read-only.  The batch is place_greedy's
        without priorities; level_size / parent describe the hierarchy exactly as for gang_capacity_tree.  The pairs
        may come in any order and repeat.  tables=False leaves the three [P] answers out (they never cross),
        first=False the per-job first fit in the caller's pair order."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        pj = _c(pair_job, np.int32).reshape(-1)
        pd = _c(pair_domain, np.int32).reshape(-1)
        if pj.shape != pd.shape:
            raise ValueError("pair_job and pair_domain must have one length")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        P = len(pj)
        fits = np.zeros(P, dtype=np.uint8) if tables else None
        fail = np.full(P, -1, dtype=np.int32) if tables else None
        pods = np.zeros(P, dtype=np.int64) if tables else None
        fst = np.full(J, -1, dtype=np.int32) if first else None
        self._chk(self.lib.pe_gang_fit_domains(self.h, J, _p(jgo), _p(cnt), _p(req), _p(nd), P, _p(pj), _p(pd), int(level),
                                               len(ls), _p(ls), _p(par), _p(fits), _p(fail), _p(pods), _p(fst)),
                  "pe_gang_fit_domains")
        return GangFit(fits, fail, pods, fst)

    def gang_preempt_domains(self, job_group_off, group_count, group_req, group_need, vic_group_off, vic_group_count,
                             vic_group_req, vic_pod_node, pair_job, pair_domain, pair_vic_off, pair_vic, level, level_size,
                             parent=None, tables=True, best=True) -> GangPreempt:
        """pe_gang_preempt_domains: for every pair p, which of its candidate victims (pair_vic[pair_vic_off[p] ..
        pair_vic_off[p + 1]), in eviction order) must go for job pair_job[p] to be placed ALONE in the level-`level`
        domain pair_domain[p]?  Phase 1 finds the smallest prefix of the list whose release places the job, phase 2
        puts back, from the end, every victim the job is placed without.  Read-only.  The incoming batch, the pairs
        and the hierarchy are gang_fit_domains'; the victims are placed gangs: their groups (vic_group_off [V + 1],
        vic_group_count, vic_group_req) and the global node id of every pod slot (vic_pod_node, -1 = skipped), as
        the placement calls return them.  tables=False leaves the three [P] answers out (they never cross),
        best=False the per-job pair with the fewest evictions."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        vgo = _c(vic_group_off, np.int32).reshape(-1)
        V = len(vgo) - 1
        vcnt = _c(vic_group_count, np.int32).reshape(-1)
        vreq = _c(vic_group_req, np.int64).reshape(-1, 4)
        vpn = None if vic_pod_node is None else _c(vic_pod_node, np.int32).reshape(-1)
        pj = _c(pair_job, np.int32).reshape(-1)
        pd = _c(pair_domain, np.int32).reshape(-1)
        if pj.shape != pd.shape:
            raise ValueError("pair_job and pair_domain must have one length")
        pvo = _c(pair_vic_off, np.int32).reshape(-1)
        if len(pvo) != len(pj) + 1:
            raise ValueError("pair_vic_off must be [P + 1]")
        pv = _c(pair_vic, np.int32).reshape(-1)
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        P = len(pj)
        prefix = np.full(P, -1, dtype=np.int32) if tables else None
        victims = np.zeros(P, dtype=np.uint64) if tables else None
        count = np.full(P, -1, dtype=np.int32) if tables else None
        bst = np.full(J, -1, dtype=np.int32) if best else None
        self._chk(self.lib.pe_gang_preempt_domains(self.h, J, _p(jgo), _p(cnt), _p(req), _p(nd), V, _p(vgo), _p(vcnt),
                                                   _p(vreq), _p(vpn), P, _p(pj), _p(pd), _p(pvo), _p(pv), int(level),
                                                   len(ls), _p(ls), _p(par), _p(prefix), _p(victims), _p(count), _p(bst)),
                  "pe_gang_preempt_domains")
        return GangPreempt(prefix, victims, count, bst)

    def _ledger(self, fn, what, gang_group_off, group_count, group_req, pod_node) -> int:
        off = _c(gang_group_off, np.int32).reshape(-1)
        cnt = _c(group_count, np.int32).reshape(-1)
        req = _c(group_req, np.int64).reshape(-1, 4)
        pod = None if pod_node is None else _c(pod_node, np.int32).reshape(-1)
        if len(off) < 1 or len(cnt) != len(req):
            raise ValueError("gang_group_off must be [V + 1], group_count and group_req one row per group")
        if pod is not None and len(pod) < int(np.clip(cnt, 0, None).astype(np.int64).sum()):
            raise ValueError("pod_node must hold one slot per pod")
        pods = ctypes.c_int64(-1)
        self._chk(fn(self.h, len(off) - 1, _p(off), _p(cnt), _p(req), _p(pod), ctypes.byref(pods)), what)
        return pods.value

    def release_gangs(self, gang_group_off, group_count, group_req, pod_node) -> int:
        """pe_release_gangs: give back what placed gangs hold.  The gangs come in the shape the placement calls take
        and return (gang_group_off [V + 1] -- a batch's job_group_off --, group_count, group_req, and pod_node = the
        global node id of every pod slot, -1 = skipped): every pod slot on a node that is not a removed slot adds its
        group's request to that node's residuals.  All-or-nothing: a call that would raise a residual above the reset
        snapshot is PE_EINVAL and changes nothing.  Works on sharded contexts (every rank makes the same call).
        Returns the number of pod slots that counted."""
        return self._ledger(self.lib.pe_release_gangs, "pe_release_gangs", gang_group_off, group_count, group_req, pod_node)

    def assume_gangs(self, gang_group_off, group_count, group_req, pod_node) -> int:
        """pe_assume_gangs: the inverse of release_gangs -- every counted pod slot takes its group's request off its
        node's residuals.  Refused (PE_EINVAL, nothing changed) when a residual would fall below 0; only these totals
        are checked, not labels, needs or the best-fit rule.  Returns the number of pod slots that counted."""
        return self._ledger(self.lib.pe_assume_gangs, "pe_assume_gangs", gang_group_off, group_count, group_req, pod_node)

    def drain_fit_domains(self, gang_group_off, group_count, group_req, group_need, pod_node, cand_node, cand_domain,
                          level, level_size, parent=None, fits=True, moved=True, fail_slot=True, target=True) -> DrainFit:
        """pe_drain_fit_domains: for every candidate c, would the pods that the book of placed gangs has on node
        cand_node[c] all find a node in the level-`level` domain cand_domain[c], the node itself taken out, and
        where?  Read-only.  The book is release_gangs' (gang_group_off [V + 1], group_count, group_req, pod_node = the
        global node id of every pod slot, -1 = skipped) plus group_need; slots on nodes that are no candidate are
        ignored.  level_size / parent describe the hierarchy exactly as for gang_capacity_tree.  Each of the four
        answers can be left out (it then never crosses).  DrainFit.move_of gives the arrays that carry a move out."""
        off = _c(gang_group_off, np.int32).reshape(-1)
        cnt = _c(group_count, np.int32).reshape(-1)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32).reshape(-1)
        pod = None if pod_node is None else _c(pod_node, np.int32).reshape(-1)
        cn = _c(cand_node, np.int32).reshape(-1)
        cd = _c(cand_domain, np.int32).reshape(-1)
        if len(off) < 1 or len(cnt) != len(req) or (nd is not None and len(nd) != len(cnt)):
            raise ValueError("gang_group_off must be [V + 1], group_count, group_req and group_need one row per group")
        if cn.shape != cd.shape:
            raise ValueError("cand_node and cand_domain must have one length")
        S = int(np.clip(cnt, 0, None).astype(np.int64).sum())
        if pod is not None and len(pod) < S:
            raise ValueError("pod_node must hold one slot per pod")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        C = len(cn)
        o_fits = np.zeros(C, dtype=np.uint8) if fits else None
        o_moved = np.zeros(C, dtype=np.int64) if moved else None
        o_fail = np.full(C, -1, dtype=np.int64) if fail_slot else None
        o_target = np.full(S, -1, dtype=np.int32) if target else None
        self._chk(self.lib.pe_drain_fit_domains(self.h, len(off) - 1, _p(off), _p(cnt), _p(req), _p(nd), _p(pod), C, _p(cn),
                                                _p(cd), int(level), len(ls), _p(ls), _p(par), _p(o_fits), _p(o_moved),
                                                _p(o_fail), _p(o_target)), "pe_drain_fit_domains")
        return DrainFit(o_fits, o_moved, o_fail, o_target)

    def scale_up_domains(self, job_group_off, group_count, group_req, group_need, tmpl_res, tmpl_labels, new_slot,
                         pair_job, pair_domain, pair_template, pair_max, level, level_size, parent=None, nodes=True,
                         fail_group=True, pods=True, new_pods=True, best=True) -> ScaleUp:
        """pe_scale_up_domains: for every pair p, the fewest nodes of template pair_template[p] (free residual
        tmpl_res[t], labels tmpl_labels[t]) that would have to join the level-`level` domain pair_domain[p] for
        place_greedy_domains to place job pair_job[p] ALONE there, trying 0, 1, ... pair_max[p] new nodes in that order
        (the answer is not monotone).  The i-th new node has id new_slot[i], a removed slot of the inventory.
        Read-only.  The batch, the pairs and the hierarchy are gang_fit_domains'; tmpl_labels None = 0, pair_max None =
        len(new_slot) for every pair.  Each of the five answers can be left out (it then never crosses)."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        tres = _c(tmpl_res, np.int64).reshape(-1, 4)
        tlab = None if tmpl_labels is None else _c(tmpl_labels, np.uint32).reshape(-1)
        if tlab is not None and len(tlab) != len(tres):
            raise ValueError("tmpl_res and tmpl_labels must have one row per template")
        slot = _c(new_slot, np.int32).reshape(-1)
        pj = _c(pair_job, np.int32).reshape(-1)
        pd = _c(pair_domain, np.int32).reshape(-1)
        pt = _c(pair_template, np.int32).reshape(-1)
        pm = None if pair_max is None else _c(pair_max, np.int32).reshape(-1)
        if pj.shape != pd.shape or pj.shape != pt.shape or (pm is not None and pm.shape != pj.shape):
            raise ValueError("pair_job, pair_domain, pair_template and pair_max must have one length")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        P = len(pj)
        o_nodes = np.full(P, -1, dtype=np.int32) if nodes else None
        o_fail = np.full(P, -1, dtype=np.int32) if fail_group else None
        o_pods = np.zeros(P, dtype=np.int64) if pods else None
        o_new = np.zeros(P, dtype=np.int64) if new_pods else None
        o_best = np.full(J, -1, dtype=np.int32) if best else None
        self._chk(self.lib.pe_scale_up_domains(self.h, J, _p(jgo), _p(cnt), _p(req), _p(nd), len(tres), _p(tres), _p(tlab),
                                               len(slot), _p(slot), P, _p(pj), _p(pd), _p(pt), _p(pm), int(level), len(ls),
                                               _p(ls), _p(par), _p(o_nodes), _p(o_fail), _p(o_pods), _p(o_new), _p(o_best)),
                  "pe_scale_up_domains")
        return ScaleUp(o_nodes, o_fail, o_pods, o_new, o_best)

    def place_first_fit_domains(self, job_group_off, priority, group_count, group_req, group_need, pair_job,
                                pair_domain, level, level_size, parent=None, pairs=True):
        """pe_place_first_fit_domains: every job, in (priority desc, index asc) order, is placed in the first of
        its candidate domains -- its pairs in ascending p, as for gang_fit_domains -- in which place_greedy_domains
        would place it against the residuals as the earlier jobs of the batch left them; a job whose candidates all
        fail, or that is in no pair, is unschedulable.  Residuals are updated in place.  Returns (pod_node,
        job_status, job_pair): job_pair[j] is the pair that placed job j or -1 (None with pairs=False)."""
        jgo = _c(job_group_off, np.int32)
        J = len(jgo) - 1
        cnt = _c(group_count, np.int32)
        req = _c(group_req, np.int64).reshape(-1, 4)
        nd = None if group_need is None else _c(group_need, np.uint32)
        pj = _c(pair_job, np.int32).reshape(-1)
        pd = _c(pair_domain, np.int32).reshape(-1)
        if pj.shape != pd.shape:
            raise ValueError("pair_job and pair_domain must have one length")
        if level_size is None:
            raise ValueError("level_size is required")
        ls = _c(level_size, np.int32).reshape(-1)
        par = None if parent is None else _c(parent, np.int32).reshape(-1)
        P = int(np.clip(cnt, 0, None).astype(np.int64).sum())
        pod = np.full(max(P, 1), -1, dtype=np.int32)
        st = np.zeros(max(J, 1), dtype=np.int32)
        jp = np.full(max(J, 1), -1, dtype=np.int32) if pairs else None
        self._chk(self.lib.pe_place_first_fit_domains(self.h, J, _p(jgo), _p(_c(priority, np.int32)), _p(cnt), _p(req),
                                                      _p(nd), len(pj), _p(pj), _p(pd), int(level), len(ls), _p(ls),
                                                      _p(par), _p(pod), _p(st), _p(jp)), "pe_place_first_fit_domains")
        return pod[:P], st[:J], (jp[:J] if pairs else None)

    # ------------------------------------------------------------ misc
    def synchronize(self):
        self._chk(self.lib.pe_synchronize(self.h), "pe_synchronize")

    def stream(self) -> int:
        return int(self.lib.pe_stream(self.h) or 0)

    def stats(self) -> dict:
        s = _abi.PeStats()
        self._chk(self.lib.pe_get_stats(self.h, ctypes.byref(s)), "pe_get_stats")
        return s.as_dict()

    def reset_stats(self):
        self._chk(self.lib.pe_reset_stats(self.h), "pe_reset_stats")


class Resolver:
    """pe_resolver_*: the host half of the windowed greedy, driven with externally supplied
    candidate blobs (one block per shard, device merge-kernel layout)."""

    def __init__(self, job_group_off, priority, group_count, group_req, group_need=None):
        self.lib = _abi.load()
        self._jgo = _c(job_group_off, np.int32)
        self.J = len(self._jgo) - 1
        self._cnt = _c(group_count, np.int32)
        self._req = _c(group_req, np.int64).reshape(-1, 4)
        self._need = None if group_need is None else _c(group_need, np.uint32)
        self.P = int(self._cnt.sum())
        h = ctypes.c_void_p()
        rc = self.lib.pe_resolver_create(self.J, _p(self._jgo), _p(_c(priority, np.int32)), _p(self._cnt),
                                         _p(self._req), _p(self._need), ctypes.byref(h))
        if rc != 0:
            raise PlacementError(rc, "pe_resolver_create")
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.pe_resolver_destroy(self.h)
            self.h = None

    def set_nodes(self, n_nodes: int):
        """pe_resolver_set_nodes: listed / seeded node ids must lie below n_nodes (PE_EINVAL otherwise)."""
        rc = self.lib.pe_resolver_set_nodes(self.h, int(n_nodes))
        if rc != 0:
            raise PlacementError(rc, "pe_resolver_set_nodes")

    def done(self) -> bool:
        return bool(self.lib.pe_resolver_done(self.h))

    def next_window(self, max_groups: int, max_pods: int) -> np.ndarray:
        out = np.zeros(max_groups, dtype=np.int32)
        n = ctypes.c_int32()
        rc = self.lib.pe_resolver_next_window(self.h, max_groups, max_pods, _p(out), ctypes.byref(n))
        if rc != 0:
            raise PlacementError(rc, "pe_resolver_next_window")
        return out[:n.value].copy()

    def resolve(self, groups: np.ndarray, blob: bytes, n_shards: int, topk: int, seeds=None):
        """seeds: [n][6] int64 {node id, res[0..3], labels} -- nodes changed since the snapshot the
        blob was scanned on, current state (pipelined form, pe_resolver_resolve_seeded)."""
        g = _c(groups, np.int32)
        buf = np.frombuffer(blob, dtype=np.uint8)
        cap = max(64, 2 * self.P + 64)
        upd = np.zeros((cap, 5), dtype=np.int64)
        nu, cons = ctypes.c_int64(), ctypes.c_int32()
        if seeds is not None and len(seeds):
            sd = _c(seeds, np.int64).reshape(-1, 6)
            rc = self.lib.pe_resolver_resolve_seeded(self.h, len(g), _p(g), _p(buf), n_shards, topk, sd.shape[0],
                                                     _p(sd), _p(upd), cap, ctypes.byref(nu), ctypes.byref(cons))
        else:
            rc = self.lib.pe_resolver_resolve(self.h, len(g), _p(g), _p(buf), n_shards, topk, _p(upd), cap,
                                              ctypes.byref(nu), ctypes.byref(cons))
        if rc != 0:
            raise PlacementError(rc, "pe_resolver_resolve")
        return upd[:nu.value].copy(), bool(cons.value)

    def results(self):
        pod = np.full(max(self.P, 1), -1, dtype=np.int32)
        st = np.zeros(max(self.J, 1), dtype=np.int32)
        self.lib.pe_resolver_results(self.h, _p(pod), _p(st))
        return pod[:self.P], st[:self.J]
