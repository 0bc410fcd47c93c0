"""Checker for pe_fit_explain: include/placement.h's rule stated twice -- cell by cell in Python integers
(explain_cells) and vectorised in numpy (explain) -- and the inputs its CPU and GPU tests share (no engine code).

    signature(j, n): bit d (0 .. 3) = req[j][d] > res[n][d] (signed), bit 4 = (labels[n] & need[j]) != need[j]
    hist[j][s] = #{live n in scope(j) : signature(j, n) == s}
    near[j][d] = min over the live n in scope(j) with signature exactly 1 << d of req[j][d] - res[n][d]; 0 if none

`res` is [4][N] as the engine holds it: a removed slot has NEVER in dimension 0 (fit_thresholds.Inventory.reference).
The scope is given as dom [N] (the node's domain at the call's level, NO_DOMAIN = none; level_domains walks the
parent map) and job_domain [J] (ANY = the whole shard); both None = every live node for every job.

explain takes wrong VARIANTS, one switch each, so that the CPU test can show that the shared inputs tell every one of
them from the rule; and `weight`, the multiplicity of each node column, so that an inventory tiled from a few distinct
rows is answered on the distinct rows alone."""
import numpy as np

import fit_thresholds as FT

D = 4
BINS = 32
LABELS = 4
ANY = -1
NO_DOMAIN = -2
NEVER = FT.NEVER
I64MAX = int(FT.I64MAX)
U64 = (1 << 64) - 1
ISLAND = FT.ISLAND
NAMES = ("cpu", "memory", "amd.com/gpu", "ephemeral-storage")

VARIANTS = ("ge", "unsigned", "zero_never", "removed_counted", "any_bit", "ignore31", "near_inclusive", "near_signed",
            "bit_order", "skip_no_island", "level0")


# ---------------------------------------------------------------- domains

def level_domains(island, level_size, parent, level):
    """[N] int32: dom_level(n) by a plain walk of the parent map, NO_DOMAIN where there is none."""
    off = [0]
    for s in level_size:
        off.append(off[-1] + int(s))
    out = np.full(len(island), NO_DOMAIN, dtype=np.int32)
    for n, isl in enumerate(np.asarray(island).tolist()):
        d = isl if 0 <= isl < level_size[0] else -1
        for l in range(level):
            if d < 0:
                break
            d = int(parent[off[l] + d])
        out[n] = d if d >= 0 else NO_DOMAIN
    return out


# ---------------------------------------------------------------- the rule, cell by cell

def explain_cells(res, labels, req, need=None, dom=None, job_domain=None):
    """(hist int64 [J][32], near uint64 [J][4]) in Python integers, one (job, node) cell at a time."""
    res = [[int(v) for v in row] for row in np.asarray(res, dtype=np.int64)]
    labels = [int(v) for v in np.asarray(labels, dtype=np.uint32)]
    req = [[int(v) for v in row] for row in np.asarray(req, dtype=np.int64).reshape(-1, D)]
    J, N = len(req), len(labels)
    need = [0] * J if need is None else [int(v) for v in np.asarray(need, dtype=np.uint32)]
    hist = np.zeros((J, BINS), dtype=np.int64)
    near = np.zeros((J, D), dtype=np.uint64)
    for j in range(J):
        best = [None] * D
        for n in range(N):
            if res[0][n] == NEVER:
                continue
            if job_domain is not None and int(job_domain[j]) != ANY and int(dom[n]) != int(job_domain[j]):
                continue
            s = 0
            for d in range(D):
                if req[j][d] > res[d][n]:
                    s |= 1 << d
            if labels[n] & need[j] != need[j]:
                s |= 1 << LABELS
            hist[j][s] += 1
            for d in range(D):
                if s == 1 << d:
                    gap = req[j][d] - res[d][n]
                    assert 1 <= gap <= U64 - 1
                    best[d] = gap if best[d] is None else min(best[d], gap)
        for d in range(D):
            near[j][d] = np.uint64(best[d] or 0)
    return hist, near


# ---------------------------------------------------------------- the rule, vectorised (and its wrong variants)

def _signed(a):
    return a.view(np.int64)


def explain(res, labels, req, need=None, dom=None, job_domain=None, weight=None, variants=(), island=None, dom0=None,
            cells=1 << 23):
    """(hist int64 [J][32], near uint64 [J][4]).  Differences are taken in uint64: req - res modulo 2^64 is the exact
    shortfall wherever req > res, so nothing can wrap.  `island` is read by the variant skip_no_island and `dom0`
    (the level-0 domains) by level0 only."""
    bad = set(variants) - set(VARIANTS)
    assert not bad, bad
    v = set(variants)
    res = np.asarray(res, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.uint32)
    req = np.ascontiguousarray(np.asarray(req, dtype=np.int64).reshape(-1, D))
    J, N = len(req), len(labels)
    need = np.zeros(J, dtype=np.uint32) if need is None else np.asarray(need, dtype=np.uint32)
    w = np.ones(N, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.int64)
    live = np.ones(N, dtype=bool) if "removed_counted" in v else res[0] != NEVER
    if "level0" in v and dom0 is not None:
        dom = dom0
    hist = np.zeros((J, BINS), dtype=np.int64)
    near = np.zeros((J, D), dtype=np.uint64)
    if N == 0 or J == 0:
        return hist, near
    step = max(1, cells // N)
    order = [(d + 1) % 5 for d in range(5)] if "bit_order" in v else list(range(5))
    for a in range(0, J, step):
        q, nd = req[a:a + step], need[a:a + step]
        B = len(q)
        scope = np.broadcast_to(live[None, :], (B, N)).copy()
        if job_domain is not None:
            jd = np.asarray(job_domain, dtype=np.int32)[a:a + step]
            scope &= (jd[:, None] == ANY) | (np.asarray(dom)[None, :] == jd[:, None])
            if "skip_no_island" in v:
                scope &= (jd[:, None] != ANY) | (np.asarray(island)[None, :] >= 0)
        elif "skip_no_island" in v:
            scope &= np.asarray(island)[None, :] >= 0
        x = []
        for d in range(D):
            qq, rr = q[:, d, None], res[d][None, :]
            if "unsigned" in v:
                qq, rr = qq.view(np.uint64), rr.view(np.uint64)
            xd = qq >= rr if "ge" in v else qq > rr
            if "zero_never" in v:
                xd = xd & (q[:, d, None] != 0)
            x.append(xd)
        n2 = nd & np.uint32(0x7FFFFFFF) if "ignore31" in v else nd
        both = labels[None, :] & n2[:, None]
        x.append((both == 0) & (n2[:, None] != 0) if "any_bit" in v else both != n2[:, None])
        sig = np.zeros((B, N), dtype=np.int64)
        for b in range(5):
            sig |= x[b].astype(np.int64) << order[b]
        idx = (np.arange(B, dtype=np.int64)[:, None] * BINS + sig)[scope]
        ww = np.broadcast_to(w[None, :], (B, N))[scope]
        hist[a:a + step] = np.bincount(idx, weights=None, minlength=B * BINS).reshape(B, BINS) if weight is None else \
            np.bincount(idx, weights=ww.astype(np.float64), minlength=B * BINS).reshape(B, BINS).astype(np.int64)
        for d in range(D):
            gap = q[:, d, None].view(np.uint64) - res[d][None, :].view(np.uint64)     # modulo 2^64
            pick = scope & (x[d] if "near_inclusive" in v else sig == (1 << order[d]))
            if "near_signed" in v:
                g = np.where(pick, _signed(gap), np.int64(I64MAX))
                m = g.min(axis=1)
                near[a:a + step, d] = np.where(pick.any(axis=1), m, 0).astype(np.int64).view(np.uint64)
            else:
                g = np.where(pick, gap, np.uint64(U64))
                near[a:a + step, d] = np.where(pick.any(axis=1), g.min(axis=1), np.uint64(0))
    return hist, near


def message(hist_row, names=NAMES):
    """The build-defined text of one job's histogram, from the rule's words alone."""
    h = [int(c) for c in hist_row]
    text = f"{h[0]}/{sum(h)} nodes are available"
    reasons = []
    for r in range(5):
        c = sum(h[s] for s in range(BINS) if s & (1 << r))
        if c and r < D:
            reasons.append(f"{c} Insufficient {names[r]}")
        elif c:
            reasons.append(f"{c} node(s) didn't match the required labels")
    return text + (": " + ", ".join(reasons) if reasons else "") + "."


# ---------------------------------------------------------------- shared inputs

class Case:
    """An inventory as the engine takes it, the batch, and (res, labels) as the engine then holds them."""

    def __init__(self, name, cap, used, labels, island, req, need, remove=()):
        self.name, self.cap, self.used, self.labels, self.island = name, cap, used, labels, island
        self.req, self.need, self.remove = req, need, np.asarray(remove, dtype=np.int64)

    def reference(self):
        res = self.cap - self.used
        lab = np.where(self.island >= 0, self.labels | ISLAND, self.labels).astype(np.uint32)
        res[:, self.remove] = NEVER
        lab[self.remove] = 0
        return res, lab


def from_rows(name, rows, labels, req, need, island=None, remove=()):
    """A case from residual rows [N][4] and node labels that may carry bit 31 (-> island = the node's own index)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, D)
    labels = np.asarray(labels, dtype=np.uint32)
    cap, used = FT.split_residual(rows.T)
    if island is None:
        island = np.where(labels & ISLAND, np.arange(len(labels)), -1).astype(np.int32)
    return Case(name, np.ascontiguousarray(cap), np.ascontiguousarray(used), (labels & ~ISLAND).astype(np.uint32),
                np.asarray(island, dtype=np.int32), np.asarray(req, dtype=np.int64).reshape(-1, D),
                np.asarray(need, dtype=np.uint32), remove)


def threshold_cases():
    """fit_thresholds.build_inventory on three batches: nodes at v - 1, v, v + 1 of every request value, label knives,
    the -1 and -INT64_MAX rows, two removable slots."""
    from placement import synth
    batches = {
        "values": FT.values_batch(9, 5, 4, 3, FT.chain_needs(4) + ((1 << 31) | 1, 1 << 31), int64max=True),
        "sweep": FT.sweep_batch(40),
        "synth": synth.make_fit_jobs(120, 11),
    }
    out = []
    for i, (name, (req, need)) in enumerate(batches.items()):
        inv = FT.build_inventory(req, need, seed=5 + i, n_diag=400)
        out.append(Case(name, inv.cap, inv.used, inv.labels, inv.island, np.asarray(req, dtype=np.int64),
                        np.asarray(need, dtype=np.uint32), inv.remove))
    return out


ARENA_SLOTS = (0, 63, 64, 255, 256, 1023, 1024, 1, 62, 65, 127, 128, 129, 191, 192, 254, 257, 319, 320, 511, 512, 513,
               767, 768, 769, 1000, 1021, 1022, 700, 701, 33, 31)


def arena():
    """One job and 1025 nodes: one node per signature at ARENA_SLOTS (wave, block and span edges), fitting filler
    elsewhere.  The node of signature s lacks one unit in every dimension s names and one label bit if s has bit 4."""
    assert len(set(ARENA_SLOTS)) == BINS and max(ARENA_SLOTS) == 1024
    req = np.array([[10, 20, 30, 40]], dtype=np.int64)
    rows = np.tile(req + 5, (1025, 1))
    labels = np.full(1025, 3, dtype=np.uint32)
    for s, slot in enumerate(ARENA_SLOTS):
        for d in range(D):
            rows[slot, d] = req[0, d] - (d + 1 if s >> d & 1 else 0)
        labels[slot] = 1 if s >> LABELS & 1 else 3
    return from_rows("arena", rows, labels, req, [3])


def near_edges():
    """Shortfalls 1, 2, 2^63 and 2^64 - 2, a tie of two nodes, and pairs of candidates that a signed minimum and an
    inclusive one order differently."""
    M = I64MAX
    rows = [(-M, M, M, M),               # a: 2^64 - 2 against cpu = INT64_MAX (g lacks ephemeral = 1 as well)
            (M, -(1 << 62), M, M),       # b: 2^63 against memory = 2^62
            (M, 1 << 62, M, M),          # h: 1 against memory = 2^62 + 1, where b lacks 2^63 + 1
            (M, M, 4, M), (M, M, 4, M),  # c, d: the tie, 1 against gpu = 5
            (M, M, M, 7), (M, M, M, 8),  # e, f: 2 and 1 against ephemeral = 9
            (3, M, M, 0),                # g: lacks cpu AND ephemeral of (4, 0, 0, 9): in no exclusive bin
            (M, M, M, M)]
    req = [(M, 0, 0, 1), (0, 1 << 62, 0, 0), (0, (1 << 62) + 1, 0, 0), (0, 0, 5, 0), (0, 0, 0, 9), (4, 0, 0, 9),
           (0, 0, 0, 0)]
    return from_rows("near", rows, np.full(len(rows), 1, dtype=np.uint32), req, np.ones(len(req), dtype=np.uint32))


def worked_example():
    """The example of include/placement.h: (rows, labels, removed slot, req, need)."""
    Gi = 1 << 30
    rows = [(8000, 128 * Gi, 8, 0), (8000, 128 * Gi, 4, 0), (2000, 32 * Gi, 0, 0), (8000, 128 * Gi, 8, 0),
            (8000, 128 * Gi, 6, 0), (8000, 128 * Gi, 8, 0)]
    return from_rows("example", rows, [1, 1, 1, 0, 1, 1], [(4000, 64 * Gi, 8, 0)], [1], remove=[5])


EXAMPLE_HIST = {0: 1, 4: 2, 7: 1, 16: 1}
EXAMPLE_NEAR = (0, 0, 2, 0)
EXAMPLE_MESSAGE = ("1/5 nodes are available: 1 Insufficient cpu, 1 Insufficient memory, 3 Insufficient amd.com/gpu, "
                   "1 node(s) didn't match the required labels.")


def tree_case(name, n, seed=9):
    """A synth inventory of n nodes under a named tree of tree_capacity, every fifth node without an island, and 40
    jobs whose requests straddle the residuals.  Returns (case, level_size, parent)."""
    import tree_capacity as TC
    from placement import synth
    inv = synth.make_inventory(n, seed)
    island, level_size, parent = TC.tree(name, n, seed)
    island = np.where(np.arange(n) % 5 == 4, -1, island).astype(np.int32)
    req, need = synth.make_fit_jobs(40, seed + 1)
    case = Case(f"{name}{n}", inv.cap, inv.used, np.asarray(inv.labels, dtype=np.uint32) & ~ISLAND, island,
                np.ascontiguousarray(req, dtype=np.int64), np.ascontiguousarray(need, dtype=np.uint32))
    return case, [int(s) for s in level_size], parent


def tiled(distinct_rows, distinct_labels, n, seed):
    """n nodes drawn from at most 128 distinct (row, label) pairs in a permuted order: (rows [n][4], labels [n],
    weight [distinct]) -- the expectation of the tiled inventory is explain(distinct, weight=weight)."""
    distinct_rows = np.asarray(distinct_rows, dtype=np.int64).reshape(-1, D)
    k = len(distinct_rows)
    assert k <= 128
    rng = np.random.default_rng(seed)
    pick = rng.permutation(np.arange(n) % k)
    return distinct_rows[pick], np.asarray(distinct_labels, dtype=np.uint32)[pick], np.bincount(pick, minlength=k)


def distinct_records(S, seed):
    """S distinct (request, need) pairs around the residuals of synth inventories: (req int64 [S][4], need [S])."""
    s = np.arange(S, dtype=np.int64)
    rng = np.random.default_rng(seed)
    req = np.stack([500 + 250 * (s % 131), (1 << 30) * (1 + s % 7), s % 9, (s // 9) * 1024], axis=1)
    need = rng.integers(0, 4, S).astype(np.uint32)
    assert len({tuple(r) for r in req.tolist()}) == S
    return np.ascontiguousarray(req), need
