"""Checker for pe_gang_slice_tree: include/placement.h's rule restated with Python integers, twice (through
tree_split.walk and tree_split.threshold), and the inputs its CPU and GPU tests share.

    z = slice_size, sl = slice_level, m = max(sl, 0), u = count // z
    the job's MIXED row: slots(l, .) for l < m (tree_capacity.tables), units(l, .) for l >= m --
        sl == NODE: units(0, k) = sum over the nodes n of leaf k of cap(j, n) // z   (gang_capacity.capacity_matrix)
        sl >= 0:    units(sl, k) = slots(sl, k) // z
        l > m:      units(l, p) = the sum of the children's units
    selection: the smallest l in [m, max_level] with a domain of units >= u, there the smallest such units, ties to
               the smallest id
    descent:   S_L = [(domain, u)]; tree_split's step on the mixed row's level l - 1 for l = L .. 1, every entry of the
               list multiplied by z when the list is S_m
"""
import numpy as np

import domain_capacity as DC
import gang_capacity as G
import tree_capacity as TC
import tree_split as TS

NODE = -1
TOO_MANY = TS.TOO_MANY
MAX_PARTS = TS.MAX_PARTS
SIZES = (1, 2, 3, 8)
FIELDS = ("level", "domain", "units", "parts", "part_domain", "part_pods", "spread")


def mixed_row(caps, slots_row, island, level_size, parent, z, sl):
    """The job's row [T] as Python integers: slots below level m, units at and above it.  caps: cap(j, n) per node
    (needed at node level only), slots_row: the job's tree_slots row."""
    off = TC.offsets(level_size)
    L = len(level_size)
    m = max(sl, 0)
    row = [int(x) for x in slots_row]
    if sl == NODE:
        leaf = [0] * level_size[0]
        for n, k in enumerate(int(x) for x in island):
            if 0 <= k < level_size[0]:
                leaf[k] += int(caps[n]) // z
        row[:off[1]] = leaf
    else:
        row[off[m]:off[m + 1]] = [x // z for x in row[off[m]:off[m + 1]]]
    par = [int(x) for x in ([] if parent is None else parent)]
    for l in range(m + 1, L):
        up = [0] * level_size[l]
        for c in range(level_size[l - 1]):
            if par[off[l - 1] + c] >= 0:
                up[par[off[l - 1] + c]] += row[off[l - 1] + c]
        row[off[l]:off[l + 1]] = up
    return row


def slice_row(row, count, z, sl, level_size, kids, max_level=None, max_parts=MAX_PARTS, step=TS.walk):
    """(level, domain, units, parts, [(leaf, pods)], spread[n_levels]) of one mixed row in plain Python."""
    off = TC.offsets(level_size)
    L = len(level_size)
    m = max(sl, 0)
    top = L - 1 if max_level is None else int(max_level)
    assert count % z == 0 and m <= top < L
    u = count // z
    level = domain = -1
    for l in range(m, top + 1):
        ok = [(row[off[l] + k], k) for k in range(level_size[l]) if row[off[l] + k] >= u]
        if ok:
            level, domain = l, min(ok)[1]
            break
    if level < 0:
        return -1, -1, 0, 0, [], [0] * L
    units = row[off[level] + domain]
    cur, spread = [(domain, u)], [0] * L
    for l in range(level, -1, -1):
        spread[l] = len(cur)
        if len(cur) > max_parts:
            return level, domain, units, TOO_MANY, [], [0] * L
        if l == m:
            cur = [(d, a * z) for d, a in cur]
        if l == 0:
            break
        nxt = []
        for p, a in cur:
            ids = kids[l][p]
            nxt += step(ids, [row[off[l - 1] + c] for c in ids], a)
        cur = nxt
    return level, domain, units, len(cur), cur, spread


class Slices:
    """The seven outputs as arrays, shaped and typed as the engine's."""

    def __init__(self, rows, max_parts, n_levels):
        J = len(rows)
        self.level = np.array([r[0] for r in rows], dtype=np.int32).reshape(J)
        self.domain = np.array([r[1] for r in rows], dtype=np.int32).reshape(J)
        self.units = np.array([r[2] for r in rows], dtype=np.int64).reshape(J)
        self.parts = np.array([r[3] for r in rows], dtype=np.int32).reshape(J)
        self.part_domain = np.full((J, max_parts), -1, dtype=np.int32)
        self.part_pods = np.zeros((J, max_parts), dtype=np.int32)
        self.spread = np.array([r[5] for r in rows], dtype=np.int32).reshape(J, n_levels)
        for j, r in enumerate(rows):
            for i, (leaf, pods) in enumerate(r[4]):
                self.part_domain[j, i], self.part_pods[j, i] = leaf, pods
        self.lists = [r[4] for r in rows]


def of_engine(got):
    """placement.TreeSlices under the checker's field names."""
    class _G:
        pass
    g = _G()
    g.level, g.domain, g.units, g.parts = got.level, got.domain, got.domain_units, got.parts
    g.part_domain, g.part_pods, g.spread = got.part_domain, got.part_pods, got.spread
    return g


def same(got, want, what="", fields=FIELDS):
    """Every cell of every output."""
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")


def consequences(row, slots_row, count, z, sl, level_size, parent, r):
    """What the header promises about one job's answer r = slice_row(...)."""
    level, domain, units, parts, lst, spread = r
    off = TC.offsets(level_size)
    L = len(level_size)
    m = max(sl, 0)
    if parts <= 0:
        assert lst == [] and spread == [0] * L and (level < 0) == (parts == 0)
        return
    assert level >= m and units >= count // z
    assert sum(n for _, n in lst) == count
    assert all(1 <= n <= int(slots_row[leaf]) for leaf, n in lst)
    assert len({leaf for leaf, _ in lst}) == len(lst) == spread[0]
    assert spread[level] == 1 and all(s == 0 for s in spread[level + 1:])
    if sl <= 0:
        assert all(n % z == 0 for _, n in lst)
    if sl == NODE:
        assert all(n // z <= row[leaf] for leaf, n in lst)
    under = dict(lst)   # pods under each domain, level by level up to sl
    for l in range(1, m + 1):
        up = {}
        for c, n in under.items():
            p = int(parent[off[l - 1] + c])
            assert p >= 0
            up[p] = up.get(p, 0) + n
        under = up
    assert all(n % z == 0 and n // z <= row[off[m] + d] for d, n in under.items())


# ---------------------------------------------------------------- cases

class Case:
    """An inventory under a hierarchy with a batch of jobs, each with its own slice size and level; rows[j] is the
    checker's mixed row, table[j] the job's tree_slots row."""

    def __init__(self, cap, used, labels, island, sizes, parent, req, need, count, z, sl, max_level, max_parts, rows, table):
        self.cap, self.used, self.labels, self.island = cap, used, labels, island
        self.sizes = list(sizes)
        self.parent = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
        self.req = np.ascontiguousarray(req, dtype=np.int64).reshape(-1, 4)
        self.need = None if need is None else np.ascontiguousarray(need, dtype=np.uint32)
        self.count = np.ascontiguousarray(count, dtype=np.int32)
        self.z = np.ascontiguousarray(z, dtype=np.int32)
        self.sl = np.ascontiguousarray(sl, dtype=np.int32)
        self.max_level = None if max_level is None else np.ascontiguousarray(max_level, dtype=np.int32)
        self.max_parts, self.rows, self.table = int(max_parts), rows, table
        self.kids = TS.children(self.sizes, self.parent)
        assert len(self.req) == len(self.count) == len(self.z) == len(self.sl) == len(rows) == len(table)

    def want_rows(self, step=TS.walk, max_parts=None, max_level="case"):
        mp = self.max_parts if max_parts is None else max_parts
        ml = self.max_level if isinstance(max_level, str) else max_level
        return [slice_row(self.rows[j], int(self.count[j]), int(self.z[j]), int(self.sl[j]), self.sizes, self.kids,
                          None if ml is None else int(ml[j]), mp, step) for j in range(len(self.count))]

    def want(self, step=TS.walk, max_parts=None, max_level="case"):
        mp = self.max_parts if max_parts is None else max_parts
        return Slices(self.want_rows(step, mp, max_level), mp, len(self.sizes))

    def split_want(self, max_parts=None):
        """tree_split.split's answer for the same counts and max_levels."""
        return TS.split(self.table, self.count, self.sizes, self.parent, self.max_level,
                        self.max_parts if max_parts is None else max_parts)


def build(cap, used, labels, eng_labels, island, sizes, parent, reqs, needs, jobs, max_parts, cache=None):
    """A Case from jobs = [(shape, units wanted, z, sl, max_level or None)]; count = units * z."""
    res = cap - used
    caps = G.capacity_matrix(res, eng_labels, reqs, needs)
    slots = TC.tables_of(caps, island, sizes, parent)[0]
    cache = {} if cache is None else cache
    rows = []
    for s, u, z, sl, ml in jobs:
        if (s, z, sl) not in cache:
            cache[(s, z, sl)] = mixed_row(caps[s], slots[s], island, sizes, parent, z, sl)
        rows.append(cache[(s, z, sl)])
    shape = np.array([j[0] for j in jobs], dtype=np.int64)
    L = len(sizes)
    ml = None if all(j[4] is None for j in jobs) else [L - 1 if j[4] is None else j[4] for j in jobs]
    reqs = np.asarray(reqs, dtype=np.int64).reshape(-1, 4)
    return Case(cap, used, labels, island, sizes, parent, reqs[shape], None if needs is None else np.asarray(needs)[shape],
                [j[1] * j[2] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs], ml, max_parts, rows, slots[shape])


def derived_units(row, slots_row, z, sl, level_size, kids, prefer=8):
    """(units wanted, max_parts) from one mixed row: 1 slice, the largest level-m domain + 1, the top domain, the top
    domain + 1 (one level: 1, the top domain and one more), a number of slices whose split needs exactly max_parts parts, one that needs max_parts + 1, and the
    smallest number of slices whose answer is not tree_split's for the same pods (z = 1 with sl <= 0, where there is
    none: 2 slices); None when the row has no such pair or no such number."""
    off = TC.offsets(level_size)
    L = len(level_size)
    m = max(sl, 0)
    top = max(row[off[L - 1]:off[L]])
    if top < 1 or (top + 1) * z >= 2**31:
        return None, None
    low_max = max(row[off[m]:off[m + 1]])
    cand = {1, low_max + 1, top, top + 1} | set(range(1, min(top, 48) + 1))
    for l in range(m, L):
        acc = 0
        for x in sorted(row[off[l]:off[l + 1]], reverse=True):
            acc += x
            cand.update((acc, acc + 1))
    by_parts = {}
    for u in sorted(x for x in cand if 1 <= x <= top):
        by_parts.setdefault(slice_row(row, u * z, z, sl, level_size, kids)[3], u)
    pairs = [p for p in by_parts if p >= 2 and p + 1 in by_parts and p < MAX_PARTS]
    if not pairs and L > 1:
        return None, None
    mp = min(pairs, key=lambda x: (abs(x - prefer), x)) if L > 1 else 1   # one level: a gang has one part or none
    other = 2
    if z > 1 or sl > 0:
        for other in sorted(x for x in cand if 1 <= x <= top + 1):
            a = slice_row(row, other * z, z, sl, level_size, kids, None, mp)
            if (a[0], a[1], a[3], a[4], a[5]) != TS.split_row(slots_row, other * z, level_size, kids, None, mp):
                break
        else:
            return None, None
    if L == 1:
        return [1, top, top + 1, other], 1
    return [1, low_max + 1, top, top + 1, by_parts[mp], by_parts[mp + 1], other], mp


_named = {}


def named_cases(name, n, shapes=10, strict=True):
    """The synth inventory of n nodes under TC.tree(name, n): one Case per (z, sl) for z in SIZES and every sl from
    NODE to n_levels - 1, all on one inventory.  Each holds every shape under the seven derived numbers of slices of
    the first shape that has them (the probe), and the probe again with max_level = m.  {(z, sl): (case, probe jobs)}.
    strict=False: an inventory on which no shape has them gets a few small numbers instead."""
    from placement import synth
    if (name, n) in _named:
        return _named[(name, n)]
    inv = synth.make_inventory(n, 7)
    island, sizes, parent = TC.tree(name, n)
    cap, used, lab, island = DC.with_islands(inv, island)
    req, need = synth.make_fit_jobs(shapes, 7 + n)
    assert not (need >> 31).any()
    caps = G.capacity_matrix(cap - used, lab, req, need)
    slots = TC.tables_of(caps, island, sizes, parent)[0]
    kids = TS.children(sizes, parent)
    out = {}
    for z in SIZES:
        for sl in range(NODE, len(sizes)):
            for probe in range(shapes):
                units, mp = derived_units(mixed_row(caps[probe], slots[probe], island, sizes, parent, z, sl), slots[probe], z, sl, sizes, kids)
                if units is not None:
                    break
            else:
                if strict:
                    raise AssertionError(f"{name} {n}: no shape spreads slices of {z} at level {sl} over max_parts and max_parts + 1 leaves")
                probe = 0   # (an inventory too small for the derived numbers: a few slices, one part at most)
                top = max(mixed_row(caps[0], slots[0], island, sizes, parent, z, sl)[TC.offsets(sizes)[-2]:])
                units, mp = [1, 2, max(top, 1), top + 1], 1
            jobs = [(s, u, z, sl, None) for s in range(shapes) for u in units] + [(probe, u, z, sl, max(sl, 0)) for u in units]
            case = build(cap, used, inv.labels, lab, island, sizes, parent, req, need, jobs, mp)
            out[(z, sl)] = (case, np.flatnonzero(np.array([j[0] for j in jobs[:shapes * len(units)]]) == probe))
    _named[(name, n)] = out
    return out


def merged(cases):
    """Several cases on one inventory as one batch (the larger max_parts)."""
    a = cases[0]
    cat = lambda f: np.concatenate([getattr(c, f) for c in cases])   # noqa: E731
    L = len(a.sizes)
    ml = np.concatenate([np.full(len(c.count), L - 1, dtype=np.int32) if c.max_level is None else c.max_level for c in cases])
    return Case(a.cap, a.used, a.labels, a.island, a.sizes, a.parent, cat("req"), None if a.need is None else cat("need"),
                cat("count"), cat("z"), cat("sl"), ml, max(c.max_parts for c in cases), sum((c.rows for c in cases), []),
                cat("table"))


def fan_case(f, kind):
    """tree_split.fan_case's inventory (fan-in f; tied, zero or distinct leaves) with slices of 1, 2 and 3 at every
    level: numbers of slices around every prefix sum of the wide parent's children that matters, and past the total."""
    base = TS.fan_case(f, kind)
    reqs = np.array([TS.GPU_REQ, [0, 0, 2, 0]], dtype=np.int64)
    lab = base.labels | np.uint32(1 << 31)
    caps = G.capacity_matrix(base.cap - base.used, lab, reqs, None)
    slots = TC.tables_of(caps, base.island, base.sizes, base.parent)[0]
    mp = max(1, min(f // 2, 64))
    jobs = []
    for z in (1, 2, 3):
        for sl in (NODE, 0, 1):
            for s in range(2):
                row = mixed_row(caps[s], slots[s], base.island, base.sizes, base.parent, z, sl)
                desc = sorted((x // z if sl == 1 else x for x in row[1:f + 1]), reverse=True)
                acc = np.cumsum(desc)
                picks = {1, desc[0], desc[0] + 1, int(acc[-1]), int(acc[-1]) + 1}
                for k in {0, 1, mp - 2, mp - 1, mp, f - 2, f - 1}:
                    if 0 <= k < f:
                        picks.update((int(acc[k]) - 1, int(acc[k]), int(acc[k]) + 1))
                jobs += [(s, u, z, sl, None) for u in sorted(x for x in picks if x >= 1)]
    return build(base.cap, base.used, base.labels, lab, base.island, base.sizes, base.parent, reqs, None, jobs, mp)


# ---------------------------------------------------------------- the hand-made traps

# (name, nodes' free GPUs, island, level_size, parent, count, z, sl, level, domain, units, parts in list order, spread)
TRAPS = [
    # (a) a block of two racks with 12 slots each: 24 slots, but 1 + 1 slices of 8 -- no fit for 3; the split by pods
    #     answers (12, 12)
    ("block_of_two_racks", [12, 12], [0, 1], [2, 1], [0, 0], 24, 8, 0, -1, -1, 0, [], [0, 0]),
    # (b) one rack of two nodes with 12 free GPUs each: 2 slices of 8 on nodes, not floor(24 / 8) = 3
    ("two_nodes_node_level", [12, 12], [0, 0], [1], None, 24, 8, NODE, -1, -1, 0, [], [0]),
    ("two_nodes_node_level_fit", [12, 12], [0, 0], [1], None, 16, 8, NODE, 0, 0, 2, [(0, 16)], [1]),
    # (c) racks with 15 and 9 slots: one slice each, the tie goes to rack 0 (best fit by slots would take rack 1)
    ("units_tie", [15, 9], [0, 1], [2, 1], [0, 0], 8, 8, 0, 0, 0, 1, [(0, 8)], [1, 0]),
    # (d) three levels, slices inside level 1: blocks with racks [5, 5] and [6, 3] hold 1 + 1 slices of 8; the 8 pods of
    #     each block are spread over its racks by slots
    ("slices_inside_blocks", [5, 5, 6, 3], [0, 1, 2, 3], [4, 2, 1], [0, 0, 1, 1, 0, 0], 16, 8, 1, 2, 0, 2,
     [(0, 5), (1, 3), (2, 6), (3, 2)], [4, 2, 1]),
    # (e) tree_split's best-fit-remainder trap in units: [10, 7, 6, 3] slices of 2, 13 wanted
    ("best_fit_last_in_units", [20, 14, 12, 6], [0, 1, 2, 3], [4, 1], [0, 0, 0, 0], 26, 2, 0, 1, 0, 26,
     [(0, 20), (3, 6)], [2, 1]),
]


def trap_case(trap):
    """A trap as a one-job case: one GPU per pod, the nodes' free GPUs as listed."""
    _, gpus, island, sizes, parent, count, z, sl = trap[:8]
    cap, used, labels, _ = TS.leaf_inventory(gpus)
    island = np.array(island, dtype=np.int32)
    return build(cap, used, labels, labels | np.uint32(1 << 31), island, sizes, parent, [TS.GPU_REQ], None,
                 [(0, count // z, z, sl, None)], 8)
