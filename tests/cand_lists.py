"""Candidate lists: the reference, the case generators and the blob reader / writer of the list-kernel tests.

A list is a CandHdr {n, flags, limit} followed by n ascending keys (pe_kernels.h); the contract is "every clean node
with key < limit is in the list".  The kernels that write lists from lists -- merge_shards_kernel, merge_ranked_kernel
(system-scope and plain loads), merge_kernel -- and empty_groups_kernel are driven by tests/cpp/cand_driver.cc, which
reads the cases written here and returns the raw output buffers; test_gpu_cand_kernels.py judges them here.

The contract, per group.  S is the multiset of keys the kernel is given, K the list length, `bound` the bound the
kernel works under (the smallest shard limit L for the shard merges, the smallest wave bound G for merge_kernel):
  sound   the keys are strictly ascending and in S, every key of S below `limit` is listed, 0 <= n <= K
  tight   with B = the keys of S below the bound: the list is the min(K, |B|) smallest of B, and
          limit = the (K+1)-th smallest of B if |B| > K, else the bound
  documented exceptions: merge_kernel with more than MG_CAP keys below G writes n = 1, the exact minimum, flags bit 0,
          limit = min + 1; a shard header with n outside [0, K] makes the merged group n = CAND_CORRUPT, limit 0; a
          nonzero xstatus word makes every group n = CAND_TIMEOUT, limit = the word
  flags   the shard merges and empty_groups: gen (0 when gen == 0); merge_kernel: the overflow bit
  bounds  nothing but a group's header and its first n key slots is written
The reference is Python integers: sort the union, cut at the bound, take K + 1.

What a generator may not do (the kernels assume it, check_preconditions asserts it for every case): each rank's list
ascending, keys unique across ranks, n <= K, every key below its own list's limit, world * K <= MG_CAP and world <= 16
for merge_shards, world <= RM_MAX_WORLD and merge_ranked_lds(world, K) <= RM_MAX_LDS for merge_ranked -- other than the
two corrupt counts (n = -1, n = K + 1) and the launches the wrappers refuse.  Every real key is >= 2^24: the key slots
past a list's n hold small poison values, which a kernel that read past n would list."""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass, field

import numpy as np

NO_KEY = (1 << 64) - 1
CAND_TIMEOUT, CAND_CORRUPT = -1, -2
MG_CAP, MG_THREADS, MG_SEL = 16384, 1024, 1024
RM_MAX_WORLD, RM_MAX_LDS = 16, 64 * 1024
MIN_KEY = 1 << 24

MERGE_SHARDS, RANKED_SYS, RANKED_PLAIN, MERGE, EMPTY = range(5)
KIND_NAMES = ("merge_shards", "ranked_sys", "ranked_plain", "merge", "empty_groups")
SHARD_KINDS = (MERGE_SHARDS, RANKED_SYS, RANKED_PLAIN)
MAGIC = 0x444E4143
FILL = 0xA5
GUARD = 4096
HIP_SUCCESS, HIP_INVALID_VALUE = 0, 1
FILLER = 0xEE          # between the slots of a rank_stride larger than a window
IN_FLAGS = 0x5A5A      # a shard header's flags: the merges do not read them


def header_constants(path):
    """The integer constants of pe_kernels.h that this file restates."""
    text = open(path).read()
    out = {}
    for name in ("MG_CAP", "MG_THREADS", "MG_SEL", "RM_MAX_WORLD", "CAND_TIMEOUT", "CAND_CORRUPT"):
        m = re.search(r"\b%s\s*=\s*(-?\d+)\s*[,;]" % name, text)
        out[name] = int(m.group(1))
    m = re.search(r"RM_MAX_LDS\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", text)
    out["RM_MAX_LDS"] = int(m.group(1)) * int(m.group(2))
    return out


def group_bytes(K):
    return 16 + 8 * K


def merge_ranked_lds(world, K):
    return (world * K + K + 1) * 8


# ---------------------------------------------------------------- cases

@dataclass
class Case:
    """One launch.  groups[g]: for a shard merge the ranks' lists [(n, limit, keys)], keys = the slot's stored keys
    (the first n are the list); for merge the wave lists [(count, bound, keys)]; for empty_groups None.
    regimes[g] (optional): (name, props) -- the topk_sort branch the group is named for (cpu test)."""
    name: str
    kind: int
    world: int          # ranks, or merge's nwaves
    K: int
    groups: list
    rank_stride: int = 0
    gen: int = 0
    xstatus: int | None = None
    refused: bool = False
    regimes: dict = field(default_factory=dict)

    @property
    def Wg(self):
        return len(self.groups)

    @property
    def id(self):
        return "%s/%s" % (KIND_NAMES[self.kind], self.name)


@dataclass
class Expect:
    n: int
    flags: int
    limit: int
    keys: list


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def tight(S, bound, K):
    """(n, limit, keys): the min(K, |B|) smallest of B = the keys of S below the bound; the (K+1)-th or the bound."""
    B = sorted(k for k in S if k < bound)
    return min(K, len(B)), (B[K] if len(B) > K else bound), B[:K]


def shard_keys(lists, K):
    """What a shard merge is given: every rank's first n keys; the smallest limit."""
    S = [k for n, _, keys in lists for k in keys[:max(0, min(n, K))]]
    return S, min(lim for _, lim, _ in lists)


def wave_keys(waves):
    S = [k for c, _, keys in waves for k in keys[:c]]
    return S, min(b for _, b, _ in waves)


def reference(case, g):
    flags = _i32(case.gen)
    if case.kind == EMPTY:
        return Expect(0, flags, NO_KEY, [])
    if case.kind == MERGE:
        S, G = wave_keys(case.groups[g])
        if sum(1 for k in S if k < G) > MG_CAP:
            return Expect(1, 1, min(S) + 1, [min(S)])
        n, limit, keys = tight(S, G, case.K)
        return Expect(n, 0, limit, keys)
    if case.xstatus:
        return Expect(CAND_TIMEOUT, flags, case.xstatus, [])
    lists = case.groups[g]
    if any(n < 0 or n > case.K for n, _, _ in lists):
        return Expect(CAND_CORRUPT, flags, 0, [])
    S, L = shard_keys(lists, case.K)
    n, limit, keys = tight(S, L, case.K)
    return Expect(n, flags, limit, keys)


def selected_keys(case, g):
    """The keys topk_sort is given for the group (those below the bound), or None where it is not reached."""
    if case.kind == MERGE:
        S, b = wave_keys(case.groups[g])
    elif case.kind == MERGE_SHARDS and not case.xstatus:
        if any(n < 0 or n > case.K for n, _, _ in case.groups[g]):
            return None
        S, b = shard_keys(case.groups[g], case.K)
    else:
        return None
    T = [k for k in S if k < b]
    return None if len(T) > MG_CAP else T


def regime(keys, K):
    """topk_sort's branch for T = len(keys) unique keys and list length K (bound NO_KEY), restated:
    ("direct" | "one" | "two" | "bitonic", the bin arithmetic that led there)."""
    T = len(keys)
    if T <= 2 * (K + 1) and T <= MG_SEL:
        return "direct", {}
    if K + 1 > MG_SEL:
        return "bitonic", {}
    kmin, kmax = min(keys), max(keys)
    bits = ((kmax - kmin) | 1).bit_length()
    sh = bits - 8 if bits > 8 else 0
    hist = [0] * 256
    for k in keys:
        hist[(k - kmin) >> sh] += 1

    def cut(h, need):   # hist_cut: the first bin whose inclusive count reaches need (255 if none), the count before it
        run = 0
        for b in range(256):
            if run + h[b] >= need:
                return b, run
            run += h[b]
        return 255, run

    cb, before = cut(hist, K + 1)
    sel_c = sum(hist[:cb + 1])
    p = {"bits": bits, "sh": sh, "cb": cb, "before": before, "sel_c": sel_c}
    if sel_c <= MG_SEL:
        return "one", p
    base = kmin + (cb << sh)
    sh2 = sh - 8 if sh > 8 else 0
    cb2 = 255
    if sh > 0:
        h2 = [0] * 256
        for k in keys:
            if (k - kmin) >> sh == cb:
                h2[(k - base) >> sh2] += 1
        cb2, _ = cut(h2, K + 1 - before)
    C = sum(1 for k in keys if (k - kmin) >> sh < cb or ((k - kmin) >> sh == cb and (k - base) >> sh2 <= cb2))
    p.update(sh2=sh2, cb2=cb2, C=C)
    return ("two" if C <= MG_SEL else "bitonic"), p


def check_preconditions(case):
    """What the kernels may assume of a case; raises AssertionError."""
    K, W = case.K, case.world
    assert K >= 1 and W >= 1 and case.Wg >= 1, case.id
    if case.kind == EMPTY:
        return
    if case.kind == MERGE:
        for waves in case.groups:
            assert len(waves) == W
            seen = set()
            for c, b, keys in waves:
                assert 0 <= c <= 64 and len(keys) == c
                assert all(MIN_KEY <= k < b for k in keys), case.id
                seen.update(keys)
            assert len(seen) == sum(c for c, _, _ in waves), case.id + ": keys repeat"
        return
    if case.refused:   # the wrapper's own check refuses the launch: nothing reaches a kernel
        assert W > RM_MAX_WORLD or merge_ranked_lds(W, K) > RM_MAX_LDS
        assert case.kind in (RANKED_SYS, RANKED_PLAIN)
    elif case.kind == MERGE_SHARDS:
        assert W <= MG_THREADS // 64 and W * K <= MG_CAP, case.id
    else:
        assert W <= RM_MAX_WORLD and merge_ranked_lds(W, K) <= RM_MAX_LDS, case.id
    assert case.rank_stride == 0 or (case.rank_stride >= case.Wg * group_bytes(K) and case.rank_stride % 8 == 0)
    corrupt = 0
    for lists in case.groups:
        assert len(lists) == W
        seen, total = set(), 0
        for n, lim, keys in lists:
            if n < 0 or n > K:
                assert n in (-1, K + 1), case.id
                corrupt += 1
            else:
                assert len(keys) == n, case.id
            assert len(keys) <= K
            assert all(a < b for a, b in zip(keys, keys[1:])), case.id + ": a list is not ascending"
            assert all(MIN_KEY <= k < lim for k in keys), case.id + ": a key at or above its list's limit"
            seen.update(keys)
            total += len(keys)
        assert len(seen) == total, case.id + ": keys repeat across ranks"
    assert corrupt <= 1, case.id


# ---------------------------------------------------------------- blobs

def input_bytes(case):
    if case.kind == EMPTY:
        return b""
    if case.kind == MERGE:
        slots = case.Wg * case.world
        cand = np.arange(1, slots * 64 + 1, dtype=np.uint64)          # poison past a list's count
        bound = np.empty(slots, dtype=np.uint64)
        cnt = np.empty(slots, dtype=np.int32)
        for g, waves in enumerate(case.groups):
            for w, (c, b, keys) in enumerate(waves):
                s = g * case.world + w
                cand[s * 64:s * 64 + c] = np.array(keys, dtype=np.uint64)
                bound[s], cnt[s] = b, c
        return cand.tobytes() + bound.tobytes() + cnt.tobytes()
    gb = group_bytes(case.K)
    window = case.Wg * gb
    stride = case.rank_stride or window
    buf = bytearray([FILLER]) * (case.world * stride + 64)   # (+64: a read of K + 1 keys of the last slot stays inside)
    for r in range(case.world):
        for g, lists in enumerate(case.groups):
            n, lim, keys = lists[r]
            slot = np.arange(1, case.K + 1, dtype=np.uint64)          # poison past n
            slot[:len(keys)] = np.array(keys, dtype=np.uint64)
            at = r * stride + g * gb
            buf[at:at + gb] = struct.pack("<iiQ", n, IN_FLAGS, lim) + slot.tobytes()
    return bytes(buf)


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(cases)))
        for c in cases:
            data = input_bytes(c)
            xs = c.xstatus if c.xstatus is not None else 0
            f.write(struct.pack("<7qQ4q", c.kind, c.world, c.Wg, c.K, c.rank_stride, c.gen, int(c.xstatus is not None), xs,
                                len(data), c.Wg * group_bytes(c.K), GUARD, 0))
            f.write(data)


def read_outputs(path, cases):
    """[(launch error, sync error, the output buffer with its guard)] per case."""
    raw = open(path, "rb").read()
    magic, n = struct.unpack_from("<II", raw, 0)
    assert magic == MAGIC and n == len(cases), (magic, n)
    at, out = 8, []
    for c in cases:
        le, se, nb = struct.unpack_from("<iiq", raw, at)
        at += 16
        assert nb == c.Wg * group_bytes(c.K) + GUARD
        out.append((le, se, raw[at:at + nb]))
        at += nb
    assert at == len(raw)
    return out


def check_output(case, result):
    """Judges one case's output against reference(); returns the list of what is wrong (empty: exact)."""
    le, se, buf = result
    gb, K, bad = group_bytes(case.K), case.K, []
    fill = bytes([FILL])
    if case.refused:
        if le != HIP_INVALID_VALUE:
            bad.append("launch error %d, expected hipErrorInvalidValue" % le)
        if buf != fill * len(buf):
            bad.append("a refused launch wrote to the output")
        return bad
    if le != HIP_SUCCESS or se != HIP_SUCCESS:
        return ["launch error %d, sync error %d" % (le, se)]
    for g in range(case.Wg):
        want = reference(case, g)
        n, flags, limit = struct.unpack_from("<iiQ", buf, g * gb)
        m = max(0, min(n, K))
        keys = list(struct.unpack_from("<%dQ" % m, buf, g * gb + 16))
        if (n, flags, limit) != (want.n, want.flags, want.limit):
            bad.append("group %d: n, flags, limit = %d, %d, %#x, expected %d, %d, %#x"
                       % (g, n, flags, limit, want.n, want.flags, want.limit))
        elif keys != want.keys:
            i = next(i for i in range(m) if keys[i] != want.keys[i])
            bad.append("group %d: key %d of %d is %#x, expected %#x" % (g, i, m, keys[i], want.keys[i]))
        rest = buf[g * gb + 16 + 8 * m:(g + 1) * gb]
        if rest != fill * len(rest):
            bad.append("group %d: key slots past n = %d were written" % (g, n))
    if buf[case.Wg * gb:] != fill * GUARD:
        bad.append("the guard behind the output was written")
    return bad


# ---------------------------------------------------------------- generators

def _rng(*seed):
    return np.random.default_rng([17, *seed])


def _unique(rng, count, lo, hi):
    """count distinct integers in [lo, hi), any width up to 64 bits."""
    out = set()
    while len(out) < count:
        need = count - len(out)
        hi_part = rng.integers(0, 1 << 32, size=need, dtype=np.uint64)
        lo_part = rng.integers(0, 1 << 32, size=need, dtype=np.uint64)
        for a, b in zip(hi_part.tolist(), lo_part.tolist()):
            out.add(lo + ((a << 32) | b) % (hi - lo))
    return sorted(out)[:count] if len(out) > count else sorted(out)


def score_keys(rng, count, id0=0):
    """count keys (score << 24) | node id with uniform 40-bit scores and ids id0, id0 + 1, ..."""
    scores = rng.integers(1, 1 << 40, size=count, dtype=np.uint64).tolist()
    return [(s << 24) | (id0 + i) for i, s in enumerate(scores)]


def deal(rng, keys, world, K):
    """The keys dealt to `world` ranks at random, as evenly as they go; every list short (limit NO_KEY)."""
    order = rng.permutation(len(keys)).tolist()
    lists = []
    for r in range(world):
        mine = sorted(keys[i] for i in order[r::world])
        assert len(mine) <= K, (len(keys), world, K)
        lists.append((len(mine), NO_KEY, mine))
    return lists


def natural(universes, K):
    """Each rank's list as an exact shard walk leaves it: the K smallest of its keys, limit = its (K+1)-th or NO_KEY."""
    lists = []
    for u in universes:
        u = sorted(u)
        lists.append((min(K, len(u)), u[K] if len(u) > K else NO_KEY, u[:K]))
    return lists


def deal_waves(rng, keys, nwaves, G=NO_KEY):
    """The keys dealt to wave lists of at most 64 in any order; every wave's bound is G."""
    order = rng.permutation(len(keys)).tolist()
    assert len(keys) <= 64 * nwaves
    waves = []
    for w in range(nwaves):
        mine = [keys[i] for i in order[w::nwaves]]
        waves.append((len(mine), G, mine))
    return waves


GRID_K = (1, 2, 63, 64, 65, 255, 1023)
GRID_WORLD = (1, 2, 3, 16)


def grid_T(K):
    return (0, 1, K, K + 1, K + 2, 2 * K + 2, 2 * K + 3)


def grid_inputs():
    """The direct-sort edge: T in {0, 1, K, K+1, K+2, 2K+2, 2K+3} keys dealt to 1, 2, 3 and 16 ranks, for every K of
    GRID_K -- every combination in which no rank needs more than K keys (T <= world * K).  One launch per (K, world),
    one group per T.  -> [(name, world, K, groups, regimes)]"""
    out = []
    for K in GRID_K:
        for world in GRID_WORLD:
            rng = _rng(1, K, world)
            groups, regimes = [], {}
            for T in grid_T(K):
                if T > world * K:
                    continue
                regimes[len(groups)] = ("direct" if T <= 2 * K + 2 and T <= MG_SEL else "not_direct", {"T": T})
                groups.append(deal(rng, score_keys(rng, T), world, K))
            out.append(("grid_K%d_w%d" % (K, world), world, K, groups, regimes))
    return out


BIN_BASE = 1 << 30
BIN_SH = 40      # key sets built on bins(): min BIN_BASE, max BIN_BASE + 2^48 - 1 -> bits 48, sh 40, bin b = offset >> 40


def bins(rng, counts, lo=None):
    """Distinct keys with counts[b] of them in first-level bin b (of the 48-bit range BIN_BASE ...), the range's two
    ends among them (bins 0 and 255 must be populated).  lo: {bin: width} keeps that bin's keys in its first `width`."""
    lo = lo or {}
    keys = set()
    for b, c in counts.items():
        start = BIN_BASE + (b << BIN_SH)
        fixed = ([BIN_BASE] if b == 0 else []) + ([BIN_BASE + (1 << 48) - 1] if b == 255 and b not in lo else [])
        got = set(fixed)
        while len(got) < c:
            got.update(_unique(rng, c - len(got), start, start + lo.get(b, 1 << BIN_SH)))
        keys |= got
    assert BIN_BASE in keys and BIN_BASE + (1 << 48) - 1 in keys
    return sorted(keys)


def spread(total, b0, b1):
    """{bin: count} of `total` keys over the bins b0 .. b1 as evenly as they go."""
    nb = b1 - b0 + 1
    counts = {b0 + i: total // nb + (i < total % nb) for i in range(nb)}
    return {b: c for b, c in counts.items() if c}


def regime_keysets():
    """The key sets named for a selection regime: (name, K, keys, (regime, props))."""
    out = []
    rng = _rng(2)
    base = 1 << 44
    # one-level cut: uniform 40-bit scores
    out.append(("one_level", 255, score_keys(rng, 16 * 255), ("one", {})))
    out.append(("one_level_16x1023", 255, score_keys(rng, 16 * 1023), ("one", {})))
    # two-level cut: a cluster spaced 2^20 apart and one key 2^40 away
    cluster = [base + (i << 20) for i in range(2400)]
    out.append(("two_level", 600, cluster + [base + (1 << 40)], ("two", {"cb": 0})))
    # bitonic fallback: the cluster as consecutive integers -- equal scores, consecutive node ids
    out.append(("bitonic", 600, [base + i for i in range(2400)] + [base + (1 << 40)], ("bitonic", {"cb": 0, "cb2": 0})))
    # shift 0: consecutive keys, one per bin
    out.append(("shift0_128", 8, [base + i for i in range(128)], ("one", {"sh": 0, "sel_c": 9})))
    out.append(("shift0_200", 8, [base + i for i in range(200)], ("one", {"sh": 0, "sel_c": 9})))
    # a key range of 2^63 or more
    wide = sorted(set(_unique(rng, 2998, MIN_KEY, NO_KEY - 1)) | {MIN_KEY, NO_KEY - 1})
    out.append(("range63", 255, wide, ("one", {"bits": 64, "sh": 56})))
    # the cut bin being bin 0 and bin 255
    out.append(("cut_bin0", 100, bins(rng, {0: 300, **spread(500, 1, 255)}), ("one", {"cb": 0, "sel_c": 300})))
    out.append(("cut_bin255", 100, bins(rng, {**spread(50, 0, 49), 255: 400}), ("one", {"cb": 255, "sel_c": 450})))
    # the (K+1)-th key the first of its bin: K keys in bin 0, the limit in bin 1
    out.append(("cut_bin_edge", 100, bins(rng, {0: 100, **spread(300, 1, 255)}), ("one", {"cb": 1, "before": 100})))
    # exactly MG_SEL and MG_SEL + 1 keys in the one-level cut
    out.append(("sel_exact", 600, bins(rng, {0: MG_SEL, **spread(400, 1, 255)}), ("one", {"cb": 0, "sel_c": MG_SEL})))
    out.append(("sel_plus1", 600, bins(rng, {0: MG_SEL + 1, **spread(400, 1, 255)}),
                ("two", {"cb": 0, "sel_c": MG_SEL + 1})))
    # the same at the second level: sub-bin 0 of bin 0 (2^32 wide) holds MG_SEL / MG_SEL + 1 keys and the (K+1)-th
    for extra, name, reg in ((0, "sel2_exact", "two"), (1, "sel2_plus1", "bitonic")):
        low = bins(rng, {0: MG_SEL + extra, 255: 1}, lo={0: 1 << 32})
        rest = bins(rng, {0: 1, **spread(400, 1, 255)})[1:]
        more = _unique(rng, 200, BIN_BASE + (1 << 33), BIN_BASE + (1 << BIN_SH))   # bin 0, later sub-bins
        out.append((name, 600, sorted(set(low) | set(rest) | set(more)), (reg, {"cb": 0, "cb2": 0, "C": MG_SEL + extra})))
    return out


def regime_cases():
    """Every named key set through merge_shards (dealt to 16 ranks, where 16 K holds it) and through merge (dealt to
    wave lists of 64).  Two of the issue's shapes hold more keys than 16 ranks of their K can list (16 x 1023 keys at K
    255, 200 keys at K 8): those run through merge_kernel, whose selection is the same topk_sort, and merge_shards gets
    the most its K admits (16 x 255, 128)."""
    out = []
    for i, (name, K, keys, reg) in enumerate(regime_keysets()):
        rng = _rng(3, i)
        if len(keys) <= 16 * K:
            out.append(Case(name, MERGE_SHARDS, 16, K, [deal(rng, keys, 16, K)], regimes={0: reg}))
        nwaves = max(4, -(-len(keys) // 60))
        out.append(Case(name, MERGE, nwaves, K, [deal_waves(rng, keys, nwaves)], regimes={0: reg}))
    return out


def grid_cases():
    """The grid through merge_shards, and through both rank merges where their LDS holds it."""
    out = []
    for name, world, K, groups, regimes in grid_inputs():
        out.append(Case(name, MERGE_SHARDS, world, K, groups, regimes=regimes))
        if merge_ranked_lds(world, K) <= RM_MAX_LDS:
            out += [Case(name, k, world, K, groups) for k in (RANKED_SYS, RANKED_PLAIN)]
    return out


def _k(x, r=0):
    return (1 << 30) + 16 * x + r      # small readable keys, unique across ranks r


def limit_groups(K=8):
    """world 3: [(what, lists)] around the smallest shard limit L."""
    r0 = [_k(10 * i) for i in range(K + 4)]            # lists 0, 10, .., 10 (K - 1); limit 10 K
    full = natural([r0], K)[0]
    short = lambda xs, r: (len(xs), NO_KEY, [_k(x, r) for x in xs])   # noqa: E731
    L = 10 * K
    g = []
    g.append(("L cuts listed keys of the other ranks",
              [full, short([5, 35, L - 5, L + 5, L + 15], 1), short([L + 10, L + 20, L + 40], 2)]))
    g.append(("L is NO_KEY, fewer than K keys", [short([1, 2, 3], 0), short([7, 9], 1), short([], 2)]))
    g.append(("L is NO_KEY, more than K keys", [short(range(0, 50, 10), 0), short(range(1, 51, 10), 1), short(range(2, 52, 10), 2)]))
    g.append(("exactly K keys below L", [full, short([L + 5, L + 15], 1), short([], 2)]))
    g.append(("exactly K + 1 keys below L", [full, short([L - 5, L + 5], 1), short([], 2)]))
    g.append(("a weak list: K - 1 keys and a real limit", [(K - 1, _k(L), r0[:K - 1]), short([L + 5], 1), short([L + 1], 2)]))
    g.append(("a listed key of another rank equals L", [(K - 2, _k(L), r0[:K - 2]), (1, NO_KEY, [_k(L)]), short([L + 1], 2)]))
    g.append(("every rank empty",[short([], 0), short([], 1), short([], 2)]))
    g.append(("an empty rank with a real limit", [(0, _k(50), []), short([20, 45, 55, 60], 1), short([30, 70], 2)]))
    g.append(("one rank holds everything", [short([], 0), (K, _k(1000, 1), [_k(10 * i, 1) for i in range(K)]), short([], 2)]))
    g.append(("every rank full, limits differ", natural([[_k(3 * i + r, r) for i in range(K + 1 + r)] for r in range(3)], K)))
    return g


def limit_cases():
    out = []
    groups = [lists for _, lists in limit_groups()]
    one = [[(0, NO_KEY, [])], [(8, _k(99), [_k(i) for i in range(8)])], [(3, NO_KEY, [_k(1), _k(5), _k(6)])],
           [(2, _k(7), [_k(1), _k(5)])]]
    for kind in SHARD_KINDS:
        out.append(Case("limits_w3", kind, 3, 8, groups))
        out.append(Case("limits_w1", kind, 1, 8, one))
    return out


def ranked_shape_groups(rng, world, K):
    """Balanced lists (the heads hold K + 1 keys: the U cut applies), one full list beside empty ones (they do not),
    disjoint ranges per rank, perfectly interleaved lists, random lists."""
    uni = lambda n, r: [(s << 24) | (r << 16) | i for i, s in   # noqa: E731
                        enumerate(rng.integers(1, 1 << 40, size=n, dtype=np.uint64).tolist())]
    g = [natural([uni(3 * K, r) for r in range(world)], K)]
    g.append(natural([uni(2 * K, r) if r == world - 1 else [] for r in range(world)], K))
    g.append(natural([[((r + 1) << 50) + (x << 8) + r for x in rng.choice(1 << 30, size=K // 2 + r, replace=False).tolist()]
                      for r in range(world)], K))
    g.append(natural([[MIN_KEY + 7 * (i * world + r) for i in range(K + 1)] for r in range(world)], K))
    g.append(natural([uni(int(rng.integers(0, 2 * K + 1)), r) for r in range(world)], K))
    return g


SEARCH_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65)


def ranked_cases():
    """merge_ranked (and merge_shards on the same input) at 1, 2, 3, 5, 8 and 16 ranks; per-rank candidate counts of
    SEARCH_COUNTS, equal and mixed, for the first step of the binary searches (K 200 at 3 ranks: the heads hold fewer
    than K + 1 keys, so every key below L is a candidate); 16 ranks at the largest K the LDS holds."""
    out = []
    for world in (1, 2, 3, 5, 8, 16):
        groups = ranked_shape_groups(_rng(4, world), world, 33)
        out += [Case("shapes_w%d" % world, k, world, 33, groups) for k in SHARD_KINDS]
    rng = _rng(5)
    mixes = [(c, c, c) for c in SEARCH_COUNTS] + [(1, 64, 5), (65, 2, 63), (3, 4, 64), (64, 0, 1), (0, 65, 0)]
    groups = []
    for mix in mixes:
        keys = score_keys(rng, sum(mix))
        order = rng.permutation(len(keys)).tolist()
        cuts = np.cumsum((0,) + mix).tolist()
        groups.append([(c, NO_KEY, sorted(keys[i] for i in order[a:a + c])) for c, a in zip(mix, cuts)])
    out += [Case("search_counts", k, 3, 200, groups) for k in SHARD_KINDS]
    big = natural([score_keys(rng, 600, id0=1000 * r) for r in range(16)], 481)
    out += [Case("w16_K481", k, 16, 481, [big]) for k in SHARD_KINDS]
    return out


def refused_cases():
    """Launches merge_ranked's wrapper refuses: 17 ranks, and one key more than the LDS holds at 16."""
    out = []
    for kind in (RANKED_SYS, RANKED_PLAIN):
        out.append(Case("w17", kind, 17, 8, [[(0, NO_KEY, [])] * 17], refused=True))
        out.append(Case("w16_K482", kind, 16, 482, [[(0, NO_KEY, [])] * 16], refused=True))
    return out


XSTATUS = (1 << 63) | (2 << 32) | 41


def every_kind_cases():
    """rank_stride larger than a window (filler between the slots), gen 0 and nonzero, one corrupt header (n = -1,
    n = K + 1) in one rank of one group, a nonzero xstatus word -- for every shard merge."""
    out = []
    K, world, Wg = 8, 3, 5
    rng = _rng(6)
    groups = [natural([score_keys(rng, int(rng.integers(0, 3 * K)), id0=100 * r) for r in range(world)], K) for _ in range(Wg)]
    wide = Wg * group_bytes(K) + 136

    def corrupt(g, r, n):
        gs = [list(lists) for lists in groups]
        _, lim, keys = gs[g][r]
        gs[g][r] = (n, lim, keys)
        return gs

    for kind in SHARD_KINDS:
        out.append(Case("gen0", kind, world, K, groups))
        out.append(Case("gen5", kind, world, K, groups, gen=5))
        out.append(Case("gen_top_bit", kind, world, K, groups, gen=0x9ABCDEF0))
        out.append(Case("stride", kind, world, K, groups, rank_stride=wide))
        out.append(Case("stride_gen", kind, world, K, groups, rank_stride=wide, gen=77))
        out.append(Case("corrupt_minus1", kind, world, K, corrupt(2, 1, -1), gen=3))
        out.append(Case("corrupt_K_plus1", kind, world, K, corrupt(1, 2, K + 1)))
        out.append(Case("corrupt_K_plus1_stride", kind, world, K, corrupt(3, 0, K + 1), rank_stride=wide, gen=4))
        out.append(Case("xstatus", kind, world, K, groups, gen=9, xstatus=XSTATUS))
        out.append(Case("xstatus_gen0", kind, world, K, groups, xstatus=XSTATUS))
        out.append(Case("xstatus_zero_word", kind, world, K, groups, gen=9, xstatus=0))
    return out


def wave_group(rng, nwaves, cut):
    """Wave lists with counts from 0 to 64 in any order.  cut: the smallest bound G lies inside the keys (wave 0 holds
    only keys below it, its bound is G; the other waves' bounds are at or above G and above their own keys)."""
    if nwaves <= 64:
        counts = rng.integers(0, 65, size=nwaves)
        counts[rng.integers(0, nwaves)] = 64
    else:   # (at most MG_CAP keys below G: mostly short lists, every tenth of any length)
        counts = np.where(rng.random(nwaves) < 0.1, rng.integers(0, 65, size=nwaves), rng.integers(0, 8, size=nwaves))
    counts = counts.tolist()
    keys = score_keys(rng, sum(counts))
    order = rng.permutation(len(keys)).tolist()
    G = NO_KEY
    if cut:
        srt = sorted(keys)
        G = srt[len(srt) // 3] + 1 if srt else MIN_KEY + 5
    waves, at = [], 0
    for w, c in enumerate(counts):
        mine = [keys[i] for i in order[at:at + c]]
        at += c
        if cut and w == 0:
            mine = [k for k in mine if k < G]
            b = G
        elif cut:
            b = max([G] + [k + 1 for k in mine]) + int(rng.integers(0, 1 << 20)) if rng.random() < 0.7 else NO_KEY
        else:
            b = NO_KEY
        waves.append((len(mine), b, mine))
    return waves


def merge_cases():
    """merge_kernel: nwaves of 1, 16, 1024, 1025 and 2000, counts from 0 to 64 per wave list in any order, bounds that
    cut; MG_CAP keys exactly (no overflow), one more and 300 full lists (overflow)."""
    out = []
    for nwaves in (1, 16, 1024, 1025, 2000):
        for K in (8, 256):
            rng = _rng(7, nwaves, K)
            groups = [wave_group(rng, nwaves, cut) for cut in (False, True, True)]
            if nwaves == 1:
                groups.append([(0, NO_KEY, [])])
                groups.append([(0, MIN_KEY + 9, [])])
            out.append(Case("waves%d_K%d" % (nwaves, K), MERGE, nwaves, K, groups))
    rng = _rng(8)
    full = score_keys(rng, 257 * 64)
    at_cap = deal_waves(rng, full[:MG_CAP], 257)
    over_by_one = deal_waves(rng, full[:MG_CAP + 1], 257)
    out.append(Case("at_cap", MERGE, 257, 8, [at_cap, over_by_one]))
    out.append(Case("overflow_300_full", MERGE, 300, 8, [deal_waves(rng, score_keys(rng, 300 * 64), 300),
                                                         deal_waves(rng, score_keys(rng, 300 * 64), 300, G=NO_KEY - 1)]))
    return out


def empty_cases():
    return [Case("Wg%d_K%d_gen%d" % (Wg, K, gen), EMPTY, 1, K, [None] * Wg, gen=gen)
            for Wg, K in ((1, 1), (5, 8), (300, 255), (3, 1023)) for gen in (0, 6, 0x80000001)]


SUITES = {
    "regimes": regime_cases,
    "grid": grid_cases,
    "limits": limit_cases,
    "ranked": ranked_cases,
    "refused": refused_cases,
    "every_kind": every_kind_cases,
    "merge": merge_cases,
    "empty": empty_cases,
}
