"""Checker for pe_gang_capacity_domains: include/placement.h's rule restated with Python integers on top of
gang_capacity.capacity_matrix (the per-node cap, true `//`), and the inputs its CPU and GPU tests share.

    dom_slots[j][k] = sum of cap(j, n) over the nodes n with island[n] == k      (0 <= k < n_domains)
    dom_nodes[j][k] = number of those nodes with cap(j, n) >= 1
    domain[j]       = the k with the smallest dom_slots[j][k] >= count[j], ties to the smallest k; -1 if none
    domain_slots[j] = that domain's slots, 0 when none      feasible[j] = #{k : dom_slots[j][k] >= count[j]}

A node whose island id is negative or >= n_domains counts nowhere (a removed slot has island -1).
`labels` are the engine's labels: synth.island_labels applied."""
import numpy as np

import gang_capacity as G
from placement import synth


def tables_of(m, island, n_domains):
    """(dom_slots int64[J][D], dom_nodes int64[J][D]) of a cap matrix m [J][N] (gang_capacity.capacity_matrix:
    Python integers): its columns grouped by island id and added up as Python integers."""
    J, N = m.shape
    island = np.asarray(island, dtype=np.int64).reshape(-1)
    assert island.shape == (N,)
    slots = np.zeros((J, n_domains), dtype=object)
    nodes = np.zeros((J, n_domains), dtype=object)
    for k in np.unique(island):
        if not 0 <= k < n_domains:
            continue
        cols = m[:, island == k]                     # object dtype: sum() adds Python integers
        slots[:, k] = cols.sum(axis=1)
        nodes[:, k] = np.asarray(cols >= 1, dtype=bool).sum(axis=1)
    assert all(0 <= int(x) < 2**63 for x in slots.reshape(-1))
    return slots.astype(np.int64), nodes.astype(np.int64)


def tables(res, labels, island, req, need, n_domains):
    """The two tables of the rule for an inventory (res [4][N], the engine's labels, island ids)."""
    return tables_of(G.capacity_matrix(res, labels, req, need), island, n_domains)


def select_row(row, count):
    """(domain, domain_slots, feasible) of one table row, in plain Python."""
    best, best_k, feasible = None, -1, 0
    for k, v in enumerate(int(x) for x in row):
        if v >= count:
            feasible += 1
            if best is None or v < best:
                best, best_k = v, k
    return best_k, (0 if best is None else best), feasible


def select(dom_slots, count):
    """(domain int32[J], domain_slots int64[J], feasible int32[J])."""
    got = [select_row(row, int(c)) for row, c in zip(dom_slots, count)]
    return (np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int64),
            np.array([g[2] for g in got], dtype=np.int32))


# ---------------------------------------------------------------- shared inputs

LAYOUTS = ("racks32", "interleaved", "one", "own", "none", "mixed")


def layout(name, n, seed=5):
    """(island int32[n], n_domains) of a named domain layout over n nodes."""
    ids = np.arange(n, dtype=np.int64)
    if name == "racks32":          # contiguous racks of 32 nodes
        return (ids // 32).astype(np.int32), (n + 31) // 32
    if name == "interleaved":      # n % D: no two neighbours share a domain
        d = max(1, min(n, 37))
        return (ids % d).astype(np.int32), d
    if name == "one":              # every node in domain 0
        return np.zeros(n, dtype=np.int32), 1
    if name == "own":              # every node its own domain
        return ids.astype(np.int32), n
    if name == "none":             # no node has a domain
        return np.full(n, -1, dtype=np.int32), 4
    if name == "mixed":            # random ids in [-2, 2D): some negative, some >= n_domains (ignored)
        d = 19
        rng = np.random.default_rng(seed + n)
        return rng.integers(-2, 2 * d, n).astype(np.int32), d
    raise ValueError(name)


def with_islands(inv, island):
    """The synth inventory with its island ids replaced: (cap, used, labels as the engine keeps them, island)."""
    island = np.asarray(island, dtype=np.int32)
    return inv.cap, inv.used, synth.island_labels(inv.labels, island), island


def special_domains():
    """gang_capacity.special_inventory() with nodes 0 and 1 sharing domain 2, node 2 alone in domain 0, node 3
    in domain 5 (outside n_domains = 4: ignored) and node 4 in no domain.  n_domains = 4."""
    cap, used, labels, _ = G.special_inventory()
    island = np.array([2, 2, 0, 5, -1], dtype=np.int32)
    return cap, used, labels, island, 4


def special_tables():
    """Per SPECIAL_CASES row the expected (dom_slots[4], dom_nodes[4]), from the hand-worked cells: domain 2
    = nodes 0 + 1, domain 0 = node 2, domains 1 and 3 empty.  A need with the island bit is met by nodes 0, 1
    and 2 here (all three have an island id >= 0), so the cells of the rows that carry it are re-worked."""
    out = []
    for q, nd, cells in G.SPECIAL_CASES:
        cells = list(cells)
        if nd & G.ISLAND:   # row ([1250, GiB, 1, 10 GiB], 1 | ISLAND): node 1 now has an island; node 2 lacks bit 0
            cells = [4, G.I63 // (10 * G.GiB), 0, 0, 0]
        out.append(([cells[2], 0, cells[0] + cells[1], 0], [int(cells[2] >= 1), 0, int(cells[0] >= 1) + int(cells[1] >= 1), 0]))
    return out
