"""Checker for pe_gang_capacity_tree: include/placement.h's rule restated with Python integers on top of
domain_capacity.tables (the leaf level), and the inputs its CPU and GPU tests share.

    level 0: tree[j][k] = dom[j][k] of pe_gang_capacity_domains with n_domains = level_size[0]
    level l + 1: tree[j][off_{l+1} + p] = sum of tree[j][off_l + c] over the c with parent[off_l + c] == p
    level[j]  = the smallest l <= max_level[j] at which some domain has slots >= count[j]; -1 if none
    domain[j] = that level's domain with the smallest such slots, ties to the smallest id; -1 if none
    domain_slots[j] = its slots, 0 when none      feasible[j][l] = #{k : slots of (l, k) >= count[j]}, every level
"""
import numpy as np

import domain_capacity as DC


def offsets(level_size):
    off = [0]
    for s in level_size:
        off.append(off[-1] + int(s))
    return off


def rollup(leaf, level_size, parent):
    """[J][T] int64 table of a leaf table [J][level_size[0]], added up with Python integers."""
    off = offsets(level_size)
    J = leaf.shape[0]
    assert leaf.shape == (J, level_size[0])
    parent = [int(x) for x in ([] if parent is None else parent)]
    assert len(parent) == off[-1] - int(level_size[-1])
    assert (np.asarray(leaf) >= 0).all()
    out = np.zeros((J, off[-1]), dtype=object)          # object dtype: += adds Python integers
    out[:, :off[1]] = np.asarray(leaf).astype(object)
    for l in range(len(level_size) - 1):
        for c in range(level_size[l]):
            p = parent[off[l] + c]
            assert -1 <= p < level_size[l + 1]
            if p >= 0:
                out[:, off[l + 1] + p] += out[:, off[l] + c]
    return out.astype(np.int64)                         # raises past int64


def tables_of(m, island, level_size, parent):
    """(tree_slots int64[J][T], tree_nodes int64[J][T]) of a cap matrix m [J][N] (gang_capacity.capacity_matrix)."""
    slots, nodes = DC.tables_of(m, island, int(level_size[0]))
    return rollup(slots, level_size, parent), rollup(nodes, level_size, parent)


def tables(res, labels, island, req, need, level_size, parent):
    slots, nodes = DC.tables(res, labels, island, req, need, int(level_size[0]))
    return rollup(slots, level_size, parent), rollup(nodes, level_size, parent)


def select_row(row, count, level_size, max_level=None):
    """(level, domain, domain_slots, feasible[n_levels]) of one table row, in plain Python."""
    off = offsets(level_size)
    L = len(level_size)
    max_level = L - 1 if max_level is None else int(max_level)
    answer, feasible = None, []
    for l in range(L):
        best, best_k, n = None, -1, 0
        for k in range(level_size[l]):
            v = int(row[off[l] + k])
            if v >= count:
                n += 1
                if best is None or v < best:
                    best, best_k = v, k
        feasible.append(n)
        if answer is None and l <= max_level and n > 0:
            answer = (l, best_k, best)
    return (answer or (-1, -1, 0)) + (feasible,)


def select(tree_slots, count, level_size, max_level=None):
    """(level int32[J], domain int32[J], domain_slots int64[J], feasible int32[J][n_levels])."""
    J = len(count)
    got = [select_row(tree_slots[j], int(count[j]), level_size, None if max_level is None else max_level[j])
           for j in range(J)]
    return (np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int32),
            np.array([g[2] for g in got], dtype=np.int64),
            np.array([g[3] for g in got], dtype=np.int32).reshape(J, len(level_size)))


# ---------------------------------------------------------------- shared inputs

TREES = ("racks32", "four", "permuted", "orphans", "childless", "fanin", "flat")
FANINS = (1, 63, 64, 65, 200)      # the group-width boundaries of one level


def _up(n, k):
    return (n + k - 1) // k


def tree(name, n, seed=9):
    """(island int32[n], level_size list, parent int32[] or None) of a named hierarchy over n nodes."""
    ids = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    if name == "racks32":          # racks of 32 nodes -> blocks of 4 racks -> one root
        r = _up(n, 32)
        b = _up(r, 4)
        return (ids // 32).astype(np.int32), [r, b, 1], np.array([k // 4 for k in range(r)] + [0] * b, dtype=np.int32)
    if name == "four":             # racks of 8 -> blocks of 4 -> zones of 3 -> root
        r = _up(n, 8)
        b = _up(r, 4)
        z = _up(b, 3)
        par = [k // 4 for k in range(r)] + [k // 3 for k in range(b)] + [0] * z
        return (ids // 8).astype(np.int32), [r, b, z, 1], np.array(par, dtype=np.int32)
    if name == "permuted":         # rack ids scattered over twice the range; children of a block anywhere
        r = _up(n, 16)
        ids0 = rng.permutation(2 * r)[:r]                    # rack i has leaf id ids0[i]: non-contiguous
        b = max(1, _up(r, 5))
        p0 = rng.integers(0, b, 2 * r)
        p1 = rng.integers(0, 2, b)
        return ids0[ids // 16].astype(np.int32), [2 * r, b, 2], np.concatenate([p0, p1]).astype(np.int32)
    if name == "orphans":          # every third rack and every other block count at their own level only
        r = _up(n, 32)
        b = _up(r, 4)
        p0 = [-1 if k % 3 == 1 else k // 4 for k in range(r)]
        p1 = [-1 if k % 2 == 1 else 0 for k in range(b)]
        return (ids // 32).astype(np.int32), [r, b, 1], np.array(p0 + p1, dtype=np.int32)
    if name == "childless":        # only the even blocks have racks; zone 1 has no block
        r = _up(n, 32)
        b = 2 * _up(r, 4) + 3
        p0 = [2 * (k // 4) for k in range(r)]
        p1 = [0 if k % 4 == 0 else 2 for k in range(b)]
        return (ids // 32).astype(np.int32), [r, b, 3], np.array(p0 + p1, dtype=np.int32)
    if name == "fanin":            # one level whose parents have 1, 63, 64, 65 and 200 children, in shuffled order
        par = np.repeat(np.arange(len(FANINS)), FANINS)
        rng.shuffle(par)
        r = len(par)               # 393 leaves; the nodes are dealt round-robin
        return (ids % r).astype(np.int32), [r, len(FANINS), 1], np.concatenate([par, np.zeros(len(FANINS))]).astype(np.int32)
    if name == "flat":             # n_levels = 1: pe_gang_capacity_domains
        return (ids // 32).astype(np.int32), [_up(n, 32)], None
    raise ValueError(name)


def fan_tree(f):
    """Two levels: parent 0 has f children (the leaves 1 .. f), parent 1 has leaf 0.  The largest fan-in, and
    so the level's group width, is set by f."""
    return [f + 1, 2], np.array([1] + [0] * f, dtype=np.int32)
