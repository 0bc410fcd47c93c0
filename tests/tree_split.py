"""Checker for pe_gang_split_tree: include/placement.h's rule restated twice with Python integers on top of
tree_capacity.tables, and the inputs its CPU and GPU tests share.

    selection: tree_capacity.select_row (pe_gang_capacity_tree's level and domain)
    descent:   S_L = [(domain, count)]; for l = L .. 1 every (P, a) of S_l in list order hands a to P's children
               (the level-(l - 1) domains c with parent[off_{l-1} + c] == P) by `step`, the results appended in order
    step `walk`:      the children sorted by (slots descending, id ascending); whole parts while slots < r, then
                      the last part r to the smallest slots >= r of the rest, ties to the smallest id
    step `threshold`: no sort of the walk -- v* = the largest child value with H(v*) >= a, the children above v*
                      and the first t equal to v* whole, the rest competing for r (the kernel's form)
    parts = |S_0| or TOO_MANY as soon as a list passes max_parts; spread[l] = |S_l|
"""
import numpy as np

import tree_capacity as TC

TOO_MANY = -1
MAX_PARTS = 1024
GPU_REQ = [0, 0, 1, 0]      # one GPU per pod: with one node per leaf, a leaf's slots are its free GPUs


def walk(ids, slots, a):
    """[(child, pods)] of allotment a over children `ids` (ascending) with `slots`: the rule as written."""
    order = sorted(range(len(ids)), key=lambda i: (-slots[i], ids[i]))
    out, r = [], a
    for pos, i in enumerate(order):
        if slots[i] >= r:
            rest = [x for x in order[pos:] if slots[x] >= r]
            last = min(rest, key=lambda x: (slots[x], ids[x]))
            return out + [(ids[last], r)]
        out.append((ids[i], slots[i]))
        r -= slots[i]
    raise AssertionError("allotment above the children's slots")


def threshold(ids, slots, a):
    """The same answer without walking a sorted list (H, G, t and r of the issue's second statement)."""
    v = max(x for x in set(slots) if x > 0 and sum(y for y in slots if y >= x) >= a)
    G = sum(y for y in slots if y > v)
    t = -(-(a - G) // v) - 1
    r = a - G - t * v
    assert 0 < r <= v
    equal = [i for i in range(len(ids)) if slots[i] == v]
    whole = [i for i in range(len(ids)) if slots[i] > v] + equal[:t]
    rest = [i for i in range(len(ids)) if i not in set(whole) and slots[i] >= r]
    last = min(rest, key=lambda i: (slots[i], ids[i]))
    whole.sort(key=lambda i: (-slots[i], ids[i]))
    return [(ids[i], slots[i]) for i in whole] + [(ids[last], r)]


def children(level_size, parent):
    """kids[l][p] = ascending level-(l - 1) ids with parent p, for l >= 1 (kids[0] is None)."""
    off = TC.offsets(level_size)
    parent = [int(x) for x in ([] if parent is None else parent)]
    kids = [None]
    for l in range(1, len(level_size)):
        lists = [[] for _ in range(level_size[l])]
        for c in range(level_size[l - 1]):
            if parent[off[l - 1] + c] >= 0:
                lists[parent[off[l - 1] + c]].append(c)
        kids.append(lists)
    return kids


def split_row(row, count, level_size, kids, max_level=None, max_parts=MAX_PARTS, step=walk):
    """(level, domain, parts, [(leaf, pods)], spread[n_levels]) of one table row in plain Python."""
    off = TC.offsets(level_size)
    L = len(level_size)
    level, domain, _, _ = TC.select_row(row, count, level_size, max_level)
    if level < 0:
        return -1, -1, 0, [], [0] * L
    cur = [(domain, int(count))]
    spread = [0] * L
    spread[level] = 1
    for l in range(level, 0, -1):
        nxt = []
        for p, a in cur:
            ids = kids[l][p]
            nxt += step(ids, [int(row[off[l - 1] + c]) for c in ids], a)
        cur = nxt
        spread[l - 1] = len(cur)
        if len(cur) > max_parts:
            return level, domain, TOO_MANY, [], [0] * L
    return level, domain, len(cur), cur, spread


class Split:
    """The six outputs as arrays, shaped and typed as the engine's."""

    def __init__(self, rows, max_parts, n_levels):
        J = len(rows)
        self.level = np.array([r[0] for r in rows], dtype=np.int32).reshape(J)
        self.domain = np.array([r[1] for r in rows], dtype=np.int32).reshape(J)
        self.parts = np.array([r[2] for r in rows], dtype=np.int32).reshape(J)
        self.part_domain = np.full((J, max_parts), -1, dtype=np.int32)
        self.part_pods = np.zeros((J, max_parts), dtype=np.int32)
        self.spread = np.array([r[4] for r in rows], dtype=np.int32).reshape(J, n_levels)
        for j, r in enumerate(rows):
            for i, (leaf, pods) in enumerate(r[3]):
                self.part_domain[j, i], self.part_pods[j, i] = leaf, pods
        self.lists = [r[3] for r in rows]


def split(tree_slots, count, level_size, parent, max_level=None, max_parts=MAX_PARTS, step=walk):
    kids = children(level_size, parent)
    rows = [split_row(tree_slots[j], int(count[j]), level_size, kids, None if max_level is None else int(max_level[j]),
                      max_parts, step) for j in range(len(count))]
    return Split(rows, max_parts, len(level_size))


FIELDS = ("level", "domain", "parts", "part_domain", "part_pods", "spread")


def same(got, want, what=""):
    """Every cell of every output."""
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {f}")


def consequences(row, count, level_size, parent, kids, r):
    """What the header promises about one job's answer r = split_row(...)."""
    level, domain, parts, lst, spread = r
    off = TC.offsets(level_size)
    L = len(level_size)
    if parts <= 0:
        assert lst == [] and spread == [0] * L
        assert (level < 0) == (parts == 0)
        return
    assert sum(n for _, n in lst) == count
    assert all(1 <= n <= int(row[leaf]) for leaf, n in lst)
    assert len({leaf for leaf, _ in lst}) == len(lst) == spread[0]
    assert spread[level] == 1 and all(s == 0 for s in spread[level + 1:])
    assert all(spread[l - 1] >= spread[l] for l in range(1, level + 1))
    if level == 0:
        assert lst == [(domain, count)]
    # allotments per level, from the leaves up; per parent the children used are the fewest that hold its allotment
    got = dict(lst)
    for l in range(1, level + 1):
        up = {}
        for c, n in got.items():
            p = int(parent[off[l - 1] + c])
            assert p >= 0
            up.setdefault(p, []).append((c, n))
        assert len(up) == spread[l]
        for p, used in up.items():
            a = sum(n for _, n in used)
            big = sorted((int(row[off[l - 1] + c]) for c in kids[l][p]), reverse=True)
            k = 1
            while sum(big[:k]) < a:
                k += 1
            assert len(used) == k, (l, p, a, used, big[:k + 1])
        got = {p: sum(n for _, n in used) for p, used in up.items()}
    assert got == {domain: count}


# ---------------------------------------------------------------- the hand-made traps

def leaf_inventory(leaf_slots):
    """(cap, used, labels, island): one node per leaf, leaf k with leaf_slots[k] free GPUs and plenty of the rest."""
    n = len(leaf_slots)
    cap = np.zeros((4, n), dtype=np.int64)
    cap[0], cap[1], cap[3] = 10**6, 10**12, 10**12
    cap[2] = np.asarray(leaf_slots, dtype=np.int64)
    return cap, np.zeros_like(cap), np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.int32)


# (name, leaf slots, level_size, parent, count, the parts in list order, spread)
TRAPS = [
    # the remainder goes to the best fit, not to the next in descending order (that would be (1, 3))
    ("best_fit_last", [10, 7, 6, 3], [4, 1], [0, 0, 0, 0], 13, [(0, 10), (3, 3)], [2, 1]),
    # ties: whole parts in id order, the remainder to the next equal child
    ("all_equal", [5, 5, 5, 5], [4, 1], [0, 0, 0, 0], 12, [(0, 5), (1, 5), (2, 2)], [3, 1]),
    # an exact fill: the last part takes a whole child, the smaller id of the two equal ones
    ("exact_fill", [8, 4, 4], [3, 1], [0, 0, 0], 12, [(0, 8), (1, 4)], [2, 1]),
    # under a grandparent: rack 0 = leaves [10, 7, 3], rack 1 = [20, 20]; the block's 43 = 40 whole + 3 to rack 0,
    # whose allotment 3 goes to its smallest leaf that holds it
    ("grandparent", [10, 7, 3, 20, 20], [5, 2, 1], [0, 0, 0, 1, 1, 0, 0], 43, [(3, 20), (4, 20), (2, 3)], [3, 2, 1]),
    # three levels: the block's 50 splits over racks 2 and 1, rack 2's 40 over two leaves; the parts of rack 2 come
    # before rack 1's although their ids are higher (worked below)
    ("list_order", [9, 30, 5, 20, 20], [5, 3, 1], [0, 1, 1, 2, 2, 0, 0, 0], 50, [(3, 20), (4, 20), (1, 10)], [3, 2, 1]),
]
# list_order, worked: racks = [9, 35, 40], the block = 84.  Count 50: no rack holds it, the block does: level 2,
# S_2 = [(0, 50)].  The racks by (slots descending, id): 2 (40), 1 (35), 0 (9).  Rack 2 is whole (40 < 50), r = 10;
# of the rest rack 1 holds 10 and rack 0 does not: S_1 = [(2, 40), (1, 10)].  Rack 2 with 40: leaf 3 whole, the
# last part 20 to leaf 4.  Rack 1 with 10: leaf 1 (30) holds it, leaf 2 (5) does not: S_0 = [(3, 20), (4, 20), (1, 10)].


def trap_tables(trap):
    _, leaf, sizes, parent, _, _, _ = trap
    return TC.rollup(np.array([leaf], dtype=np.int64), sizes, parent)


# ---------------------------------------------------------------- counts derived from the checker's own table

def derived_counts(row, level_size, parent, prefer=8):
    """(counts, max_parts) for one table row of a multi-level case, so that under max_parts the row's jobs show:
    count 1, the largest leaf slots + 1, the top domain's slots, the top domain's slots + 1 (no level holds
    it), a count whose split needs exactly max_parts parts and one that needs max_parts + 1.  max_parts is the
    m >= 2 closest to `prefer` for which both exist; None when the row has no such pair."""
    off = TC.offsets(level_size)
    L = len(level_size)
    kids = children(level_size, parent)
    row = [int(x) for x in row]
    top = max(row[off[L - 1]:off[L]])
    assert top == max(row) and top + 1 < 2**31, "the top level's largest domain is the largest of all"
    leaf_max = max(row[:off[1]])
    cand = {1, leaf_max + 1, top, top + 1}
    for l in range(L):   # prefix sums of each level's descending slots, and their neighbours
        acc = 0
        for x in sorted(row[off[l]:off[l + 1]], reverse=True):
            acc += x
            cand.update((acc, acc + 1))
    by_parts = {}
    for c in sorted(x for x in cand if 1 <= x <= top):
        by_parts.setdefault(split_row(row, c, level_size, kids)[2], c)
    pairs = [m for m in by_parts if m >= 2 and m + 1 in by_parts and m < MAX_PARTS]
    if not pairs:
        return None, None
    m = min(pairs, key=lambda x: (abs(x - prefer), x))
    return np.array([1, leaf_max + 1, top, top + 1, by_parts[m], by_parts[m + 1]], dtype=np.int32), m


def probe_row(tree_slots, level_size, parent, prefer=8):
    """The first row of a table that derived_counts accepts: (row index, counts, max_parts)."""
    off = TC.offsets(level_size)
    for j in range(tree_slots.shape[0]):
        row = tree_slots[j]
        top = int(row[off[-2]:].max())
        if top != int(row.max()) or top + 1 >= 2**31 or top <= int(row[:off[1]].max()):
            continue
        counts, m = derived_counts(row, level_size, parent, prefer)
        if counts is not None:
            return j, counts, m
    raise AssertionError("no row of the table spreads a gang over max_parts and max_parts + 1 leaves")


# ---------------------------------------------------------------- shared cases

class Case:
    """An inventory under a hierarchy with a batch of jobs; `table` is the checker's tree_slots per job."""

    def __init__(self, cap, used, labels, island, sizes, parent, req, need, count, max_level, max_parts, table):
        self.cap, self.used, self.labels, self.island = cap, used, labels, island
        self.sizes, self.parent = list(sizes), parent
        self.req = np.ascontiguousarray(req, dtype=np.int64).reshape(-1, 4)
        self.need = None if need is None else np.ascontiguousarray(need, dtype=np.uint32)
        self.count = np.ascontiguousarray(count, dtype=np.int32)
        self.max_level = None if max_level is None else np.ascontiguousarray(max_level, dtype=np.int32)
        self.max_parts, self.table = int(max_parts), table
        assert len(self.req) == len(self.count) == table.shape[0]

    def want(self, step=walk, max_parts=None):
        return split(self.table, self.count, self.sizes, self.parent, self.max_level,
                     self.max_parts if max_parts is None else max_parts, step)


_named = {}


def named_case(name, n, shapes=10, strict=True):
    """The synth inventory of n nodes under TC.tree(name, n) with `shapes` pod shapes.  Multi-level: every shape
    under each of the six counts derived from the probe row (derived_counts), then the probe shape again under
    each count with max_level 0 and 1.  One level (`flat`): the counts 1, the largest leaf and one more."""
    from placement import synth
    import domain_capacity as DC
    if (name, n) in _named:
        return _named[(name, n)]
    inv = synth.make_inventory(n, 7)
    island, sizes, parent = TC.tree(name, n)
    cap, used, lab, island = DC.with_islands(inv, island)
    req, need = synth.make_fit_jobs(shapes, 7 + n)
    assert not (need >> 31).any()
    tab = TC.tables(cap - used, lab, island, req, need, sizes, parent)[0]
    if len(sizes) == 1:
        big = int(tab[tab < 2**31 - 1].max())
        counts, m, probe = np.array([1, max(big, 1), big + 1], dtype=np.int32), 1, 0
    else:
        try:
            probe, counts, m = probe_row(tab, sizes, parent)
        except AssertionError:
            if strict:
                raise
            big = int(tab[tab < 2**31 - 1].max())
            probe, counts, m = 0, np.array([1, 2, max(big, 1), big + 1], dtype=np.int32), 1
    C = len(counts)
    shape = np.concatenate([np.repeat(np.arange(shapes), C), np.full(2 * C, probe)])
    count = np.concatenate([np.tile(counts, shapes), counts, counts])
    max_level = np.concatenate([np.full(shapes * C, len(sizes) - 1), np.zeros(C), np.full(C, min(1, len(sizes) - 1))])
    c = Case(cap, used, inv.labels, island, sizes, parent, req[shape], need[shape], count, max_level, m, tab[shape])
    c.probe = np.flatnonzero(shape[:shapes * C] == probe)   # the probe shape's jobs under the top max_level
    _named[(name, n)] = c
    return c


FAN_KINDS = ("tied", "zero", "distinct")


def fan_case(f, kind):
    """TC.fan_tree(f) with one node per leaf: leaf 0 alone under parent 1, the leaves 1 .. f under parent 0 with
    tied slots (all 5), slots with zeros between (0, 3, 3, 0, 7, ...) or distinct ones (a permutation of 1 .. f).
    Two shapes, one and two GPUs per pod; counts around every prefix sum that matters and past the total."""
    sizes, parent = TC.fan_tree(f)
    rng = np.random.default_rng(100 + f)
    if kind == "tied":
        kid = np.full(f, 5)
    elif kind == "zero":
        kid = np.resize(np.array([0, 3, 3, 0, 7, 1, 0, 3]), f)
        kid[-1] = 4
    else:
        kid = rng.permutation(f) + 1
    leaf = np.concatenate([[2], kid]).astype(np.int64)
    cap, used, labels, island = leaf_inventory(leaf)
    reqs = np.array([GPU_REQ, [0, 0, 2, 0]], dtype=np.int64)
    tab = TC.tables(cap - used, labels | np.uint32(1 << 31), island, reqs, None, sizes, parent)[0]
    m = max(1, min(f // 2, 64))
    shape, count = [], []
    for s in range(2):
        desc = np.sort(tab[s, 1:f + 1])[::-1]
        acc = np.cumsum(desc)
        picks = {1, int(desc[0]), int(desc[0]) + 1, int(acc[-1]), int(acc[-1]) + 1}
        for k in {0, 1, m - 2, m - 1, m, f - 2, f - 1}:
            if 0 <= k < f:
                picks.update((int(acc[k]) - 1, int(acc[k]), int(acc[k]) + 1))
        for c in sorted(x for x in picks if x >= 1):
            shape.append(s)
            count.append(c)
    shape = np.array(shape)
    return Case(cap, used, labels, island, sizes, parent, reqs[shape], None, count, None, m, tab[shape])


def trap_case(trap):
    """A hand-made trap as a one-job case: one node per leaf, one GPU per pod."""
    _, leaf, sizes, parent, count, _, _ = trap
    cap, used, labels, island = leaf_inventory(leaf)
    tab = TC.tables(cap - used, labels | np.uint32(1 << 31), island, [GPU_REQ], None, sizes, parent)[0]
    return Case(cap, used, labels, island, sizes, np.array(parent, dtype=np.int32), [GPU_REQ], None, [count], None, 8, tab)


# ---------------------------------------------------------------- the wide hierarchy of the chunk and slice test

def split_wide(table, shape, count, level_size, parent, max_level, max_parts):
    """split() for tables too wide and batches too long for a Python loop over every column: job j reads row
    table[shape[j]]; the selection per level is numpy's (int64 compares and argmin, exact); the descent is the
    plain walk over a parent's children WITH slots (a child without slots is never reached by the walk: every
    allotment is >= 1), listed once per row.  test_tree_split_cpu.py holds it to split()."""
    off = TC.offsets(level_size)
    L = len(level_size)
    kids = [None] + [[np.array(k, dtype=np.int64) for k in lists] for lists in children(level_size, parent)[1:]]
    live = {}

    def with_slots(s, l, p):
        if (s, l, p) not in live:
            k = kids[l][p]
            v = table[s, off[l - 1] + k]
            live[(s, l, p)] = (k[v > 0].tolist(), v[v > 0].tolist())
        return live[(s, l, p)]

    rows = []
    for j in range(len(count)):
        s, c = int(shape[j]), int(count[j])
        row = table[s]
        level = domain = -1
        for l in range(L if max_level is None else int(max_level[j]) + 1):
            seg = row[off[l]:off[l + 1]]
            ok = seg >= c
            if ok.any():
                level, domain = l, int(np.where(ok, seg, np.iinfo(np.int64).max).argmin())   # the first of equals
                break
        if level < 0:
            rows.append((-1, -1, 0, [], [0] * L))
            continue
        cur, spread = [(domain, c)], [0] * L
        spread[level] = 1
        for l in range(level, 0, -1):
            nxt = []
            for p, a in cur:
                nxt += walk(*with_slots(s, l, p), a)
            cur = nxt
            spread[l - 1] = len(cur)
            if len(cur) > max_parts:
                break
        rows.append((level, domain, TOO_MANY, [], [0] * L) if len(cur) > max_parts else (level, domain, len(cur), cur, spread))
    return Split(rows, max_parts, L)
