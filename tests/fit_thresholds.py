"""Inputs and reference of the fit-threshold suite: nodes on both sides of every request value (no engine code).

The fit mask asks, per (job, node), `(labels & need) == need` and `req_d <= res_d` in the four dimensions.  Every
kernel route answers through an encoding of the node against the BATCH -- ranks against its sorted values, digits of
those ranks, shifted and saturated residuals, guard-bit fields -- so an inventory bites only where its residuals lie
between the batch's values.  This module builds such inventories from a batch:

  fit_rows / fit_packed   the reference: numpy int64 comparisons only, no arithmetic, hence exact
  threshold_inventory     knife nodes at v - 1, v, v + 1 of every value of every dimension, diagonal nodes with all
                          four dimensions at a threshold at once, label knives, specials, shuffled
  coverage / assert_covered   what the inventory reaches, computed from inputs and reference alone
  values_batch, i32_batch, i32_nodes, sweep_batch, digit_boundary_ranks   batches and nodes for the builders' seams
  rank_table              the ranks the earlier fit tests' own inventories reach"""
from typing import NamedTuple

import numpy as np

D = 4
I64MAX = np.iinfo(np.int64).max
NEVER = np.iinfo(np.int64).min           # a removed slot's residual
I32MAX = (1 << 31) - 1
ISLAND = np.uint32(1 << 31)              # PE_NEED_ISLAND: label bit 31 = the node has an island
DIMS = ("cpu", "memory", "gpu", "ephemeral")


# ---------------------------------------------------------------- reference

def fit_rows(res, labels, req, need):
    """[J][N] bool: job j fits node n.  Comparisons only."""
    res = np.asarray(res, dtype=np.int64)
    req = np.asarray(req, dtype=np.int64).reshape(-1, D)
    labels = np.asarray(labels, dtype=np.uint32)
    need = np.asarray(need, dtype=np.uint32)
    fit = (labels[None, :] & need[:, None]) == need[:, None]
    for d in range(D):
        fit &= req[:, d, None] <= res[d][None, :]
    return fit


def pack_rows(fit):
    """The uint64 rows pe_fit_mask_rows returns: bit n % 64 of word n / 64 of row j, padding bits zero."""
    J, N = fit.shape
    by = np.packbits(fit, axis=1, bitorder="little")
    out = np.zeros((J, (N + 63) // 64 * 8), dtype=np.uint8)
    out[:, :by.shape[1]] = by
    return out.view("<u8").astype(np.uint64, copy=False)


def fit_packed(res, labels, req, need, cells=1 << 25):
    """(rows uint64 [J][ceil(N / 64)], counts int64 [J]) of fit_rows, a band of jobs at a time."""
    req = np.asarray(req, dtype=np.int64).reshape(-1, D)
    need = np.asarray(need, dtype=np.uint32)
    J, N = len(req), np.asarray(res).shape[1]
    rows = np.zeros((J, (N + 63) // 64), dtype=np.uint64)
    counts = np.zeros(J, dtype=np.int64)
    step = max(1, cells // max(N, 1))
    for a in range(0, J, step):
        f = fit_rows(res, labels, req[a:a + step], need[a:a + step])
        rows[a:a + step] = pack_rows(f)
        counts[a:a + step] = f.sum(axis=1)
    return rows, counts


def node_ranks(values, res_d):
    """#{v <= residual} against the sorted distinct values: the rank every encoding starts from."""
    return np.searchsorted(np.asarray(values, dtype=np.int64), np.asarray(res_d, dtype=np.int64), side="right")


# ---------------------------------------------------------------- the threshold inventory

class Inventory(NamedTuple):
    cap: np.ndarray        # [4][N] int64, >= 0
    used: np.ndarray       # [4][N] int64, >= 0: residual = cap - used
    labels: np.ndarray     # [N] uint32 without bit 31
    island: np.ndarray     # [N] int32: >= 0 where the node's label bit 31 is to be set
    remove: np.ndarray     # the two slots the test removes with PE_NODE_REMOVE after loading
    knife_dim: np.ndarray  # [N] the knife node's dimension, -1 for every other node
    knife_delta: np.ndarray   # [N] -1, 0, +1: the knife node sits at value + delta

    def arrays(self):
        return self.cap, self.used, self.labels, self.island

    def residual(self):
        return self.cap - self.used

    def node_labels(self):
        return np.where(self.island >= 0, self.labels | ISLAND, self.labels).astype(np.uint32)

    def reference(self):
        """(res, labels) as the engine holds them once `remove` is gone."""
        res, lab = self.residual(), self.node_labels()
        res[:, self.remove] = NEVER
        lab[self.remove] = 0
        return res, lab


def split_residual(res):
    """cap, used >= 0 with cap - used = res: a negative residual is cap 0, used -r."""
    res = np.asarray(res, dtype=np.int64)
    return np.where(res >= 0, res, 0), np.where(res < 0, -res, 0)


def foreign_bits(needs):
    """Up to three label bits (16 .. 30) no need of the batch asks for."""
    every = int(np.bitwise_or.reduce(needs)) if len(needs) else 0
    free = [b for b in range(16, 31) if not every >> b & 1][:3]
    assert free, "every label bit 16 .. 30 is needed by the batch"
    return np.uint32(sum(1 << b for b in free))


def build_inventory(req, need, seed, n_diag=1000):
    req = np.asarray(req, dtype=np.int64).reshape(-1, D)
    need = np.asarray(need, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    vals = [np.unique(req[:, d]) for d in range(D)]
    top = np.array([v[-1] for v in vals], dtype=np.int64)
    needs = np.unique(need)
    every = np.uint32(np.bitwise_or.reduce(needs))
    foreign = foreign_bits(needs)
    res_parts, lab_parts, kd_parts, kdelta_parts = [], [], [], []

    def add(r, lab, kdim=-1, kdelta=0):
        r = np.asarray(r, dtype=np.int64).reshape(-1, D)
        res_parts.append(r)
        lab_parts.append(np.broadcast_to(np.asarray(lab, dtype=np.uint32), (len(r),)).copy())
        kd_parts.append(np.full(len(r), kdim, dtype=np.int32))
        kdelta_parts.append(np.full(len(r), kdelta, dtype=np.int32))

    # knife nodes: one dimension at v - 1, v, v + 1, the others at their largest request, every need satisfied
    for d in range(D):
        for delta in (-1, 0, 1):
            v = vals[d][vals[d] < I64MAX] if delta == 1 else vals[d]
            r = np.tile(top, (len(v), 1))
            r[:, d] = v + delta
            add(r, every, d, delta)
    # diagonal nodes: every dimension at a random value of the batch - 1, + 0 or + 1
    r = np.empty((n_diag, D), dtype=np.int64)
    for d in range(D):
        v = vals[d][rng.integers(0, len(vals[d]), n_diag)]
        dl = rng.integers(-1, 2, n_diag)
        r[:, d] = v + np.where((v == I64MAX) & (dl == 1), 0, dl)
    base = needs[rng.integers(0, len(needs), n_diag)]
    mode = rng.integers(0, 4, n_diag)
    part = base & rng.integers(0, 1 << 32, n_diag, dtype=np.uint64).astype(np.uint32)
    lab = np.where(mode < 2, every, np.where(mode == 2, base | foreign, part))
    add(r, lab.astype(np.uint32))
    # label knives: exactly s, s with each one of its bits cleared, s plus foreign bits (and plus bit 31)
    for s in needs:
        short = [s & ~np.uint32(1 << b) for b in range(32) if int(s) >> b & 1]
        labs = [s] + short + [s | foreign, s | foreign | ISLAND]
        add(np.tile(top, (len(labs), 1)), np.array(labs, dtype=np.uint32))
    # specials (the all-INT64_MAX node goes last, below); the last two rows here are the removable slots
    add(np.zeros(D, dtype=np.int64), every)
    for d in range(D):
        r = top.copy()
        r[d] = -1
        add(r, every)
    add(np.full(D, -I64MAX, dtype=np.int64), every)
    n = sum(len(p) for p in res_parts) + 3
    if n % 64 == 0:
        add(top, every)
    add(np.tile(top, (2, 1)), every)
    res = np.concatenate(res_parts)
    lab = np.concatenate(lab_parts)
    kd = np.concatenate(kd_parts)
    kdelta = np.concatenate(kdelta_parts)
    # shuffle: neighbouring ranks spread over lanes, words and blocks
    perm = rng.permutation(len(res))
    remove = np.sort(np.flatnonzero(np.isin(perm, [len(res) - 2, len(res) - 1])))
    res, lab, kd, kdelta = res[perm], lab[perm], kd[perm], kdelta[perm]
    res = np.concatenate([res, np.full((1, D), I64MAX, dtype=np.int64)])
    lab = np.concatenate([lab, np.array([0xFFFFFFFF], dtype=np.uint32)])
    kd = np.concatenate([kd, [-1]]).astype(np.int32)
    kdelta = np.concatenate([kdelta, [0]]).astype(np.int32)
    N = len(res)
    assert N % 64
    cap, used = split_residual(res.T)
    island = np.where(lab & ISLAND, np.arange(N), -1).astype(np.int32)
    return Inventory(np.ascontiguousarray(cap), np.ascontiguousarray(used), (lab & ~ISLAND).astype(np.uint32), island,
                     remove, kd, kdelta)


def threshold_inventory(req, need, seed, n_diag=1000):
    """(cap, used, labels, island) for the batch; build_inventory gives the same with the removable slots named."""
    return build_inventory(req, need, seed, n_diag).arrays()


# ---------------------------------------------------------------- what an inventory reaches

def coverage(res, labels, req, need):
    """From inputs and reference alone.  Per dimension: `m` distinct request values and `ranks`, the set of node
    ranks #{v <= residual}; `knife[d][i]`: for value i of dimension d a job asking it, a node at v and a node at
    v - 1 exist such that both nodes pass the job's labels and other dimensions -- the dimension alone decides.
    `needs[s]` = (exact, one bit short, superset): a node with exactly the labels s; for EVERY bit of s a node that
    lacks only that bit; a node with s and more -- each with room for a job that needs s.  `last_fits`: the last node
    fits some job; `zero_blocked`: the all-zero request does not fit every node."""
    res = np.asarray(res, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.uint32)
    req = np.asarray(req, dtype=np.int64).reshape(-1, D)
    need = np.asarray(need, dtype=np.uint32)
    out = {"m": [], "ranks": [], "knife": [], "needs": {}}
    needs, need_ix = np.unique(need, return_inverse=True)
    lab_ok = (labels[None, :] & needs[:, None]) == needs[:, None]
    for d in range(D):
        vals, first = np.unique(req[:, d], return_index=True)
        out["m"].append(len(vals))
        out["ranks"].append(np.unique(node_ranks(vals, res[d])))
        knife = np.zeros(len(vals), dtype=bool)
        order = np.argsort(res[d], kind="stable")
        sorted_res = res[d][order]
        for i, (v, j) in enumerate(zip(vals, first)):
            pair = []
            for x in (v, v - 1):
                lo, hi = np.searchsorted(sorted_res, x, "left"), np.searchsorted(sorted_res, x, "right")
                cand = order[lo:hi]
                if not len(cand):
                    break
                ok = lab_ok[need_ix[j]][cand]
                for e in range(D):
                    if e != d:
                        ok = ok & (res[e][cand] >= req[j, e])
                pair.append(ok.any())
            knife[i] = len(pair) == 2 and all(pair)
        out["knife"].append(knife)
    for k, s in enumerate(needs):
        j = int(np.flatnonzero(need_ix == k)[0])
        room = np.ones(len(labels), dtype=bool)
        for d in range(D):
            room &= res[d] >= req[j, d]
        lacking = np.uint32(s) & ~labels
        short = all((room & (lacking == np.uint32(1 << b))).any() for b in range(32) if int(s) >> b & 1)
        out["needs"][int(s)] = (bool((room & (labels == s)).any()), bool(short),
                                bool((room & (lacking == 0) & (labels != s)).any()))
    out["last_fits"] = bool(fit_rows(res[:, -1:], labels[-1:], req, need).any())
    zero = np.zeros((1, D), dtype=np.int64)
    out["zero_blocked"] = not fit_rows(res, labels, zero, np.zeros(1, dtype=np.uint32)).all()
    return out


def assert_covered(cov, what=""):
    """The conditions every batch of the GPU suite is held to."""
    for d in range(D):
        m = cov["m"][d]
        if m >= 2:
            assert len(cov["ranks"][d]) == m + 1, (what, DIMS[d], len(cov["ranks"][d]), m + 1)
        lone = np.flatnonzero(~cov["knife"][d])
        assert not len(lone), (what, DIMS[d], "values without a knife pair", lone[:8])
    for s, (exact, short, more) in cov["needs"].items():
        assert exact and short and more, (what, hex(s), exact, short, more)
    assert cov["last_fits"], (what, "the last node fits no job")
    assert cov["zero_blocked"], (what, "the all-zero request fits every node")


# ---------------------------------------------------------------- batches for the builders' seams

CHAIN3 = (0, 1, 1 | (1 << 31))                       # an inclusion chain the coded paths take
ANTICHAIN = (0, 1, 2)                                # 1 and 2: neither holds the other
SPECIAL_VALUES = (0, 1 << 32, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, (1 << 32) + 1)
FILL = ((100, 37), (1 << 20, 3), (1, 7), (7 << 10, 5))      # field f's further values: a * (i + 1) + b


def value_table(f, k, int64max=False):
    """k distinct non-negative values of field f: 0 first, then the values around 2^31 and 2^32 (the one-set plane
    encoder carries a value as two 32-bit halves) as far as k reaches, then a * (i + 1) + b; INT64_MAX on request."""
    a, b = FILL[f]
    t = list(SPECIAL_VALUES) + [a * (i + 1) + b for i in range(k)]
    t = t[:k]
    if int64max and k > 1:
        t[-1] = I64MAX
    assert len(set(t)) == k and min(t) >= 0
    return np.array(t, dtype=np.int64)


def chain_needs(n):
    """n label needs forming an inclusion chain: 0, bit 0, bits 0-1, ..."""
    return tuple((1 << i) - 1 for i in range(n))


def values_batch(k_cpu, k_mem, k_gpu, k_eph, needs, int64max=False):
    """Job j takes value j % k_f of field f and need j % len(needs); J is the largest count, rounded up until J - 1 is
    no multiple of 16 (hence none of 64)."""
    ks = (k_cpu, k_mem, k_gpu, k_eph)
    J = max(ks + (len(needs),))
    while (J - 1) % 16 == 0:
        J += 1
    j = np.arange(J)
    req = np.stack([value_table(f, ks[f], int64max and f == 1)[j % ks[f]] for f in range(D)], axis=1)
    need = np.array(needs, dtype=np.uint32)[j % len(needs)]
    return np.ascontiguousarray(req), need


def i32_batch(s, kind):
    """Requests for the 32-bit compare's seams, the same in all four dimensions but for the multiplier.  `max`: the
    largest request is exactly INT32_MAX << s, the shift stays s; `over`: 2^31 << s, the shift becomes s + 1 and
    every request is a multiple of 2^(s + 1); `odd`: as `over` with one request that is not, so the batch must run on
    the int64 compare."""
    unit = 1 << (s + 1)
    base = [0, unit, 3 * unit, 1000 * unit, (1 << 30) << s]
    top = I32MAX << s if kind == "max" else (1 << 31) << s
    rows = []
    for d in range(D):
        col = base + [top]
        if kind == "odd":
            col[1] = unit + (1 << s)
        rows.append(np.roll(np.array(col * 3, dtype=np.int64), d)[:17])
    req = np.ascontiguousarray(np.stack(rows, axis=1))
    req[16] = 0
    need = np.array(CHAIN3, dtype=np.uint32)[np.arange(17) % 3]
    return req, need


def i32_nodes(s):
    """Residuals on the saturation line of shift s and s + 1, each again with every bit below the shift set, and the
    negative ones that tell floor from truncation and -1 from 0: rows of [4] with the same value everywhere."""
    low = (1 << (s + 1)) - 1
    edge = [I32MAX << s, (I32MAX << s) + 1, ((1 << 31) << s) - 1, (1 << 31) << s, (I32MAX << (s + 1)), (1 << 32) << s]
    vals = edge + [v | low for v in edge] + [-1, -(1 << s), -(1 << s) - 1, -(1 << (s + 1)), -(1 << (s + 1)) - 1, 0, low]
    return np.tile(np.array(vals, dtype=np.int64)[:, None], (1, D))


def with_nodes(inv, rows, labels):
    """`inv` with further nodes (residual rows [n][4]) put in front of its last one."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, D)
    res = np.concatenate([inv.residual()[:, :-1], rows.T, inv.residual()[:, -1:]], axis=1)
    lab = np.concatenate([inv.node_labels()[:-1], np.full(len(rows), labels, dtype=np.uint32), inv.node_labels()[-1:]])
    pad = np.full(len(rows), -1, dtype=np.int32)
    kd = np.concatenate([inv.knife_dim[:-1], pad, inv.knife_dim[-1:]])
    kdelta = np.concatenate([inv.knife_delta[:-1], pad * 0, inv.knife_delta[-1:]])
    if res.shape[1] % 64 == 0:
        return with_nodes(inv, np.concatenate([rows, rows[-1:]]), labels)
    cap, used = split_residual(res)
    island = np.where(lab & ISLAND, np.arange(len(lab)), -1).astype(np.int32)
    return Inventory(np.ascontiguousarray(cap), np.ascontiguousarray(used), (lab & ~ISLAND).astype(np.uint32), island,
                     inv.remove, kd, kdelta)


def sweep_batch(m, ballast=(0, 0, 0)):
    """The LDS level sweep: cpu has m values (the field under test), memory one (folded), gpu two and ephemeral three
    (crossed).  `ballast` gives memory, gpu and ephemeral storage that many values instead (0: as before): further
    fields that take planes out of the block's budget, so that the cpu field has to go to two or three levels at a
    few values, where the planner's own base divides m, instead of at hundreds or 10^5."""
    b_mem, b_gpu, b_eph = ballast
    J = max(m, *ballast)
    j = np.arange(J)
    req = np.empty((J, D), dtype=np.int64)
    req[:, 0] = 5 + 10 * (j % m)
    req[:, 1] = (1 << 30) + ((j % b_mem) * 4096 + 1 if b_mem else 0)
    req[:, 2] = j % (b_gpu or 2)
    req[:, 3] = (j % b_eph) * 4096 + 1 if b_eph else (j % 3) << 30
    need = (j % 2).astype(np.uint32)
    return req, need


def digit_boundary_ranks(m, B, L, n_edge, n_random, seed):
    """Node ranks 0 .. m on digit boundaries: t * B^k + {-1, 0, +1} for k = 1 .. L - 1, the first and last n_edge
    ranks, and random ones."""
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, n_edge), np.arange(m - n_edge, m + 1), rng.integers(0, m + 1, n_random)]
    for k in range(1, L):
        p = B ** k
        t = np.arange(0, m // p + 1) * p
        if len(t) > 3 * n_edge:                      # (level 1 of a large field: a random share of its multiples)
            t = np.concatenate([t[:n_edge], t[-n_edge:], rng.choice(t, n_edge, replace=False)])
        parts += [t - 1, t, t + 1]
    r = np.concatenate(parts)
    return r[(r >= 0) & (r <= m)]


def residual_of_rank(values, rank, rng):
    """A residual whose rank against the sorted distinct `values` is `rank`: the value itself or, where the gap to
    the next allows, a point inside the gap; below the first value for rank 0."""
    values = np.asarray(values, dtype=np.int64)
    rank = np.asarray(rank)
    lo = np.where(rank > 0, values[np.maximum(rank, 1) - 1], values[0] - 1)
    hi = np.where(rank < len(values), values[np.minimum(rank, len(values) - 1)], lo + 2)     # exclusive
    inside = np.where((rank > 0) & (hi - lo > 1) & (rng.integers(0, 2, len(rank)) == 1), 1, 0)
    return lo + inside * np.minimum(hi - lo - 1, 1 + rng.integers(0, 3, len(rank)))


def digits(rank, B, L):
    """[L][n]: digit k of each rank, base B below the top level, the top level whatever is left."""
    rank = np.asarray(rank, dtype=np.int64)
    return np.stack([rank // B ** k % B if k < L - 1 else rank // B ** k for k in range(L)])


# ---------------------------------------------------------------- the gap this suite closes, as a table

def rank_table():
    """Markdown rows: distinct node ranks out of the m + 1 possible, per dimension, that the inventories of the
    earlier fit tests reach with their own generators and seeds (no kernel involved)."""
    import test_gpu_lds as TL
    from placement import synth

    def row(name, res, req):
        cells = []
        for d in (0, 1, 3):
            vals = np.unique(req[:, d])
            cells.append(f"{len(np.unique(node_ranks(vals, res[d])))} / {len(vals) + 1}")
        return f"| {name} | " + " | ".join(cells) + " |"

    out = ["| test | cpu | memory | ephemeral |", "|---|---|---|---|"]
    for shape in ("adversarial", "unique_mem", "wide"):
        req = TL.batch(shape, 1500, 12)[0]
        out.append(row(f"`test_lds_shapes_vs_oracle[{shape}]`", TL.inventory(20011, 6).residual(), req))
    rng = np.random.default_rng(23)
    req, _ = synth.make_fit_jobs(700, 23)
    req[:, 0] = rng.integers(1, 151, 700) * 100
    req[:, 1] = rng.integers(1, 151, 700) * (1 << 26)
    req[:, 3] = rng.integers(0, 100, 700) * (1 << 30)
    out.append(row("`test_lds_level_counts`", TL.inventory(9000, 21).residual(), req))
    rng = np.random.default_rng(75)
    req, _ = synth.make_fit_jobs(60000, 75)
    for d, scale in ((0, 1), (1, 1 << 20), (3, 7)):
        req[:, d] = scale * (1 + rng.permutation(60000))
    out.append(row("`test_lds_four_level_fields` (W = 2)", TL.inventory(6001, 73).residual(), req))
    inv = synth.make_inventory(1_000_000, synth.SEED["cfg5"], 0.2)
    req, _ = synth.make_fit_jobs_worst(100_000, synth.SEED["cfg5"], (0, 1, 3))
    out.append(row("`test_lds_full_size_worst_case` (1M x 100k)", inv.residual(), req))
    inv = synth.make_inventory(5000, 71 + 5000, 0.5)
    inv.cap[1, ::7] = 1 << 50
    inv.used[0, 3::11] = inv.cap[0, 3::11] + 1000
    out.append(row("`test_fit_mask_paths` (5000 x 300)", inv.residual(), synth.make_fit_jobs(300, 373)[0]))
    return "\n".join(out)


# ---------------------------------------------------------------- the suite's named batches

# (cpu, memory, gpu, ephemeral value counts, needs) on both sides of build_codes' seams; test_gpu_fit_thresholds
# derives the path each must take from fit_encodings.coded_plan
CODED_SEAMS = {
    "therm31": ((8, 8, 5, 7), CHAIN3),                    # 8 + 8 + 5 + 7 + 3 = 31 bits: the thermometer's last
    "therm32": ((8, 8, 6, 7), CHAIN3),                    # 32: SWAR fields
    "swar_k3": ((3, 2, 2, 2), CHAIN3), "swar_k4": ((4, 2, 2, 2), CHAIN3),
    "swar_k7": ((7, 2, 2, 2), CHAIN3), "swar_k8": ((8, 2, 2, 2), CHAIN3),
    "swar_k15": ((2, 15, 2, 2), CHAIN3), "swar_k16": ((2, 16, 2, 2), CHAIN3),
    "swar_k127": ((127, 2, 2, 2), CHAIN3), "swar_k128": ((128, 2, 2, 2), CHAIN3),     # CODE_MAXV refuses 128
    "word32": ((127, 127, 63, 31), CHAIN3),               # 8 + 8 + 7 + 6 + 3 = 32 bits
    "word33": ((127, 127, 63, 63), CHAIN3),               # 8 + 8 + 7 + 7 + 3 = 33
    "needs4": ((3, 3, 2, 2), chain_needs(4)),             # the need field grows a bit at 4 needs
    "antichain": ((3, 3, 2, 2), ANTICHAIN),
    "int64max": ((5, 9, 2, 3), CHAIN3),                   # memory's largest value is INT64_MAX
}
# (value counts, needs): 32 pairs in all are one plane set, 33 are not
PLANE_SEAMS = {
    "pairs32_one_field": ((28, 1, 1, 1), (0,)),           # one field takes 28 of the 32
    "pairs32": ((8, 8, 8, 5), CHAIN3),
    "pairs33": ((29, 1, 1, 1), (0,)),                     # sets: the first closes with exactly 32 planes
    "pairs33_spread": ((8, 8, 8, 6), CHAIN3),
    "sets_close_at_31": ((29, 29, 1, 1), (0,)),           # two fields move together: 31 planes, the next job 33
    "sets_full_twice": ((57, 1, 1, 1), (0,)),             # 28 + 28 + 1 cpu values: two sets full, one of 5 planes
}
I32_SEAMS = [(s, kind) for s in (0, 6) for kind in ("max", "over", "odd")]


def path_batches():
    """The batch kinds of test_gpu_mask_device.PATHS and the adversarial LDS batch."""
    import test_gpu_lds as TL
    import test_gpu_mask_device as MD
    return {"cfg5": MD.make_batch("cfg5", 130, 141), "chain": MD.make_batch("chain", 130, 143),
            "many": MD.make_batch("many", 300, 145), "adversarial": TL.batch("adversarial", 1500, 12)}


def seam_batch(name):
    if name in CODED_SEAMS or name in PLANE_SEAMS:
        ks, needs = (CODED_SEAMS.get(name) or PLANE_SEAMS[name])
        return values_batch(*ks, needs, int64max=name == "int64max")
    raise KeyError(name)


def seam_inventory(name, req, need, seed=7):
    """The threshold inventory of a seam batch; a few hundred diagonal nodes are enough for these."""
    return build_inventory(req, need, seed, n_diag=300)


def i32_case(s, kind, seed=9):
    req, need = i32_batch(s, kind)
    inv = with_nodes(build_inventory(req, need, seed, n_diag=300), np.concatenate([i32_nodes(s), i32_nodes(s + 1)]),
                     0xFFFFFFFF)
    return req, need, inv


# ---------------------------------------------------------------- which faults the earlier inputs let through

def mutant_record():
    """Markdown rows: per mutant of fit_encodings, the inputs of test_gpu_lds.py and test_fit_mask_paths (their own
    generators and seeds) on which the mutated encoding still equals the reference -- a record, nothing asserted."""
    import fit_encodings as FE
    import test_gpu_lds as TL
    from placement import synth

    inputs = {}
    inv = TL.inventory(20011, 6)
    for shape in ("cpu400", "unique_mem", "wide", "adversarial", "needs", "extremes"):
        inputs[f"lds[{shape}]"] = (inv.residual(), inv.labels) + TL.batch(shape, 1500, 12)
    inv = synth.make_inventory(5000, 71 + 5000, 0.5)
    inv.cap[1, ::7] = 1 << 50
    inv.used[0, 3::11] = inv.cap[0, 3::11] + 1000
    inputs["paths[5000x300]"] = (inv.residual(), inv.labels) + synth.make_fit_jobs(300, 373)
    want = {k: fit_rows(*v) for k, v in inputs.items()}
    out = ["| mutant | emulated as | not distinguished by |", "|---|---|---|"]

    def row(mutant, how, fn):
        blind, n = [], 0
        for k, v in inputs.items():
            got = fn(*v)
            if got is None:
                continue
            n += 1
            if np.array_equal(got, want[k]):
                blind.append(k)
        out.append(f"| `{mutant}` | {how} | {len(blind)} of {n}: {', '.join(blind) or '-'} |")

    for mu in FE.MUTANTS["digit"]:
        L = 1 if mu == "base_off" else 2
        row(mu, f"digit planes, {L} level{'s' * (L > 1)}", lambda *a, mu=mu, L=L: FE.lds_fit(*a, levels=L, mutant=mu))
    for mu in FE.MUTANTS["i32"]:
        row(mu, "32-bit compare", lambda *a, mu=mu: FE.i32_fit(*a, mutant=mu))
    row("narrow", "SWAR code word", lambda *a: FE.coded_fit(*a, no_therm=True, mutant="narrow"))
    row("therm_no_minus", "thermometer code word", lambda *a: FE.coded_fit(*a, mutant="therm_no_minus"))
    return "\n".join(out)
