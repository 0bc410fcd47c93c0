"""The int64 edges of the PodGroup aggregation (pe_pg_min_resources, _keys, _wide): hand-built jobs on
both sides of every step of agg_job_t (training-operator_amd/csrc/pe_kernels.hip) at which an add_ovf or
mul_ovf sits, the batches that carry them down every call path and request packing, and a restatement of
the rule with switches that each make it subtly wrong.  Test code, no engine code.

  table(s, wide)     the cases of one value grid: every request cell is m << s with m < 2^32 (a narrowed
                     segment's form), or any int64 (`wide`).  Each step comes as a pair: the largest value
                     the grid allows that stays in int64 (flag 0) and the first one out (flag 1), values
                     worked out by hand as Python ints.
  edge_batch(...)    the table of each key's grid as one key-table batch: key d's cells lie on shift sh[d],
                     the edge in key d of its own jobs, ordinary values in the other keys.
  model(...)         agg_job_t restated in wrapped int64 arithmetic, from packed (narrowed) cells when asked,
                     recording the step that first left int64; FAULTS are its switches.
  narrowable / saves_bytes   the packing rule of narrow_seg (pe_engine.cpp) restated.
  assemble(...)      edge jobs among filler at chosen lanes of the planner's segments (plan restated).

Two facts of the engine the batches rely on: narrowing ORs ALL cells of a key, present or not, so one
absent cell spanning more than 32 bits keeps every segment that holds it wide; and PE_AGG_WIDE,
PE_AGG_CHUNKS, PE_AGG_THREADS, PE_AGG_ONE_PLAN and PE_AGG_NO_NT are read once per process, so packing is
steered through the data, never through them."""
from __future__ import annotations

import numpy as np

import wide_agg as WA
from agg_batches import one_job_csr, random_keys_csr
from wide_agg import C_, INIT, KIND_SHIFT, OVER, RMAX, SIDE, V1, V2

LIM = 1 << 63
U64 = (1 << 64) - 1
M32 = (1 << 32) - 1
SHIFTS = (0, 1, 30, 31, 32, 33, 61, 62)
WIDE_CELL = 1 | 1 << 40            # spans 41 bits: under a clear presence bit it only stops the narrowing
STEPS = ("main", "side", "over", "init", "side+main", "pod+over", "mul", "acc")
SUM_STEPS = STEPS[:6]              # sums inside one pod: within reach of <= 4 cells only from shift 30 on


class A(int):
    """A cell value under a CLEAR presence bit."""


def mant_bits(s, wide):
    return 63 if wide else min(32, 63 - s)


def parts(T, s, wide):
    """T >= 0 (a multiple of the grid unit) as the fewest (at least two, if T allows) grid cells."""
    cap = (1 << mant_bits(s, wide)) - 1
    sh = 0 if wide else s
    M = T >> sh
    assert M << sh == T
    n = min(max(2, -(-M // cap)), max(M, 1))
    assert n <= 4, (T, s)
    base, rem = divmod(M, n)
    return [(base + (i < rem)) << sh for i in range(n)]


def table(s, wide=False):
    """-> list of dicts: name, step, side ('in' | 'out' | 'one'), mode, job (min_member, [(replicas,
    [(kind, cell | None | A(cell))])]) over ONE key, want (the exact value, past int64 too), flag, mem
    (members), pres (key present), kabs (|multiplier| between the deciding step and the cells)."""
    u = 1 if wide else 1 << s
    mb = mant_bits(s, wide)
    sums = wide or s >= 30
    sh = 0 if wide else s
    pt = lambda T: parts(T, s, wide)                      # noqa: E731
    cs = lambda kind, vs: [(kind, v) for v in vs]         # noqa: E731
    big_cell = ((1 << mb) - 1) << sh                      # the largest cell of the grid
    big = LIM - u if sums else big_cell                   # the largest pod within reach
    sm = lambda n: n << sh if n < 1 << mb and (n << sh) * 16 < LIM else 0   # noqa: E731  (a small value)
    T = []

    def add(name, step, side, mode, job, want, flag, mem=None, pres=True, kabs=1):
        if mem is None:
            assert mode == V2                             # (the replica sum, wrapped to int32 like Go's)
            mem = ((sum(r for r, _ in job[1]) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        T.append(dict(name=name, step=step, side=side, mode=mode, job=job, want=want, flag=flag, mem=mem,
                      pres=pres, kabs=kabs))

    v2 = lambda groups: (0, groups)                       # noqa: E731
    # ---- the sums inside one pod, to LIM - u and to LIM
    if sums:
        for tgt, side, flag in ((LIM - u, "in", 0), (LIM, "out", 1)):
            p = pt(tgt)
            add("main", "main", side, V2, v2([(1, cs(C_, p))]), tgt, flag)
            add("side", "side", side, V2, v2([(1, cs(SIDE, p))]), tgt, flag)
            add("over", "over", side, V2, v2([(1, cs(OVER, p))]), tgt, flag)
            # side + v of an init container; out: the wrapped sum is negative, the max discards it, flag stays
            add("init", "init", side, V2, v2([(1, cs(SIDE, p[:-1]) + [(INIT, p[-1])])]), tgt, flag)
            add("side+main", "side+main", side, V2, v2([(1, [(C_, p[0])] + cs(SIDE, p[1:]))]), tgt, flag)
            add("pod+over", "pod+over", side, V2, v2([(1, [(INIT, p[0])] + cs(OVER, p[1:]))]), tgt, flag)
            w = u if p[0] > u else 0
            add("pod+over beside a smaller main", "pod+over", side, V2,
                v2([(1, [(INIT, p[0]), (C_, w)] + cs(OVER, p[1:]))]), tgt, flag)
    # ---- the max against initmax: pairs that differ in one bit only, both orders
    base = (6 if mb >= 3 else 2 if mb == 2 else 0) << sh
    lo_bit = 1 << sh
    hi_bit = 1 << 40 if wide else (1 << 31) << s if mb == 32 and s >= 1 else None
    for bit, nm in ((lo_bit, "bit 0"), (hi_bit, "a bit above 31")):
        if bit is None:
            continue
        add(f"max: init larger in {nm}", "max", "one", V2, v2([(1, [(INIT, base | bit), (C_, base)])]), base | bit, 0)
        add(f"max: main larger in {nm}", "max", "one", V2, v2([(1, [(INIT, base), (C_, base | bit)])]), base | bit, 0)
    if not wide and s == 0:                               # cells below 2^32: bit 32 only through a sum
        add("max: main larger in a bit above 31", "max", "one", V2,
            v2([(1, [(INIT, 7), (C_, 1 << 31), (C_, (1 << 31) + 7)])]), (1 << 32) + 7, 0)
    if mb >= 3:
        add("overhead added after the max", "max", "one", V2,
            v2([(3, [(INIT, base | lo_bit), (C_, base), (OVER, lo_bit)])]), 3 * ((base | lo_bit) + lo_bit), 0)
    # ---- pod x k
    add("k = 1, the largest pod", "mul", "one", V2, v2([(1, cs(C_, pt(big)))]), big, 0)
    r_in = (LIM - 1) // RMAX // u * u                     # (2^32 + 2) (2^31 - 1) = 2^63 - 2
    for P, side, flag in ((r_in, "in", 0), (r_in + u, "out", 1)):
        add("k = 2^31 - 1", "mul", side, V2, v2([(RMAX, cs(C_, pt(P)))]), P * RMAX, flag, kabs=RMAX)
    add("k = 0 with a huge pod", "mul", "one", V2, v2([(0, cs(C_, pt(big)))]), 0, 0)
    add("k = -1", "mul", "one", V2, v2([(-1, cs(C_, pt(big)))]), -big, 0)
    n_in = (1 << 32) // u * u                             # 2^32 x -2^31 = -2^63 exactly
    for P, side, flag in ((n_in, "in", 0), (n_in + u, "out", 1)):
        add("k = -2^31", "mul", side, V2, v2([(-(1 << 31), cs(C_, pt(P)))]), -P << 31, flag, kabs=1 << 31)
    # ---- acc + t across groups
    X = r_in * RMAX
    if sums:
        for tgt, side, flag in ((LIM - u, "in", 0), (LIM, "out", 1)):
            add("acc up", "acc", side, V2, v2([(1, [(C_, v)]) for v in pt(tgt)]), tgt, flag)
        for tgt, side, flag in ((LIM, "in", 0), (LIM + u, "out", 1)):
            add("acc down", "acc", side, V2, v2([(-1, [(C_, v)]) for v in pt(tgt)]), -tgt, flag)
        lower = [(-(1 << 31), cs(C_, pt(1 << 32)))] if wide or s <= 32 else [(-1, [(C_, v)]) for v in pt(LIM)]
        add("-2^63 then + the largest pod", "acc", "one", V2, v2(lower + [(1, cs(C_, pt(LIM - u)))]), -u, 0)
        p = pt(LIM)
        add("overflow, then back in range: sticky", "acc", "out", V2,
            v2([(1, [(C_, v)]) for v in p] + [(-1, [(C_, p[-1])]), (1, [(C_, 0)])]), LIM - p[-1], 1)
    else:                                                 # shifts 0 and 1: near 2^63 only through products
        w_in = (LIM - 1 - X) // u * u
        for w, side, flag in ((w_in, "in", 0), (w_in + u, "out", 1)):
            add("acc up", "acc", side, V2, v2([(RMAX, cs(C_, pt(r_in))), (1, [(C_, w)])]), X + w, flag)
        d0 = ((1 << 32) - u) << 31                        # -d0 = -2^63 + u 2^31
        for w, side, flag in ((u << 31, "in", 0), ((u << 31) + u, "out", 1)):
            add("acc down", "acc", side, V2, v2([(-(1 << 31), cs(C_, pt((1 << 32) - u))), (-1, [(C_, w)])]),
                -d0 - w, flag)
        add("-2^63 then + the largest product", "acc", "one", V2,
            v2([(-(1 << 31), cs(C_, pt(1 << 32))), (RMAX, cs(C_, pt(r_in)))]), X - LIM, 0)
        add("overflow, then back in range: sticky", "acc", "out", V2,
            v2([(RMAX, cs(C_, pt(r_in))), (1, [(C_, w_in + u)]), (-1, [(C_, w_in + u)]), (1, [(C_, 0)])]), X, 1)
    # ---- V2 members: Go's int32 wrap (groups without containers)
    for name, reps, mem in (("wraps once", [RMAX, RMAX], -2), ("wraps twice", [RMAX] * 4, -4),
                            ("wraps once, negative", [-(1 << 31), -(1 << 31), -1], -1),
                            ("wraps twice, negative", [-(1 << 31)] * 4 + [-7], -7),
                            ("exactly 2^31 - 1", [1 << 30, (1 << 30) - 1], RMAX),
                            ("exactly -2^31", [-(1 << 30), -(1 << 30)], -(1 << 31))):
        add("members " + name, "members", "one", V2, v2([(r, []) for r in reps]), 0, 0, mem=mem, pres=False)
    # ---- V1: the min_member cut
    c5, c3, c7 = sm(5), sm(3), sm(7)
    for mm in (RMAX, 1, 0, -1, -(1 << 31)):
        k1 = max(0, min(3, mm))
        k2 = max(0, min(2, mm - k1))
        add(f"v1 min_member {mm}", "v1", "one", V1, (mm, [(3, [(C_, c5)]), (2, [(C_, c3)])]), c5 * k1 + c3 * k2, 0,
            mem=k1 + k2, pres=k1 > 0)
    add("v1 cut on the first pod of a group", "v1", "one", V1,
        (4, [(3, [(C_, c5)]), (5, [(C_, c3)]), (2, [(C_, c7)])]), 3 * c5 + c3, 0, mem=4)
    add("v1 cut on the last pod of a group", "v1", "one", V1,
        (8, [(3, [(C_, c5)]), (5, [(C_, c3)]), (2, [(C_, c7)])]), 3 * c5 + 5 * c3, 0, mem=8)
    add("v1 groups with replicas <= 0 between counted ones", "v1", "one", V1,
        (10, [(2, [(C_, c5)]), (0, cs(C_, [big_cell] * 2)), (-1, cs(C_, [big_cell] * 2)), (2, [(C_, c3)])]),
        2 * c5 + 2 * c3, 0, mem=4)
    add("v1 min_member 0 before a huge group", "v1", "one", V1, (0, [(RMAX, cs(C_, [big_cell] * 2))]), 0, 0,
        mem=0, pres=False)
    add("v1 min_member 1 of 2^31 - 1 huge pods", "v1", "one", V1, (1, [(RMAX, cs(C_, pt(big)))]), big, 0, mem=1)
    for P, side, flag in ((r_in, "in", 0), (r_in + u, "out", 1)):
        add("v1 min_member 2^31 - 1, all counted", "v1 room", side, V1, (RMAX, [(RMAX, cs(C_, pt(P)))]), P * RMAX,
            flag, mem=RMAX, kabs=RMAX)
    c_in = (LIM - 1) // (1 << 30) // u * u                # in range only because of the cut
    for P, side, flag in ((c_in, "in", 0), (c_in + u, "out", 1)):
        add("v1 product cut to room", "v1 room", side, V1, (1 << 30, [(RMAX, cs(C_, pt(P)))]), P << 30, flag,
            mem=1 << 30, kabs=1 << 30)
        add("v1 product of a whole group, the next one cut", "v1 r", side, V1,
            ((1 << 30) + 1, [(1 << 30, cs(C_, pt(P))), (5, [])]), P << 30, flag, mem=(1 << 30) + 1,
            kabs=1 << 30)
    # ---- presence
    add("present with value 0", "presence", "one", V2, v2([(2, [(C_, 0)])]), 0, 0)
    add("present only in records v1 ignores", "presence", "one", V1, (3, [(2, [(INIT, c5), (OVER, c3), (C_, None)])]),
        0, 0, mem=2, pres=False)
    add("absent with a nonzero cell", "presence", "one", V2, v2([(2, [(C_, A(big_cell))])]), 0, 0, pres=False)
    add("absent with a nonzero cell beside a present one", "presence", "one", V2,
        v2([(2, [(C_, A(big_cell)), (C_, c3)])]), 2 * c3, 0)
    add("v1 present with value 0", "presence", "one", V1, (5, [(2, [(C_, 0)])]), 0, 0, mem=2)
    add("v1 absent with a nonzero cell", "presence", "one", V1, (5, [(2, [(C_, A(big_cell))])]), 0, 0, mem=2,
        pres=False)
    return T


# --------------------------------------------------------------------------- batches

def _other(d, ci, sh):
    """An ordinary value of another key on its own grid (small enough for any multiplier), always present."""
    return ((ci % 3) + 1) << sh[d] if sh[d] <= 24 else 0


def expand(case, n_keys, e, sh, wide, pad=0):
    """A one-key case as a job of n_keys keys with the edge in key e -> (job for WA.build with the absent
    cells as None, [(container of the job, key, cell)] to write afterwards)."""
    mm, groups = case["job"]
    out, patches, ci = [], [], 0
    pad = max(pad, 1 if wide else 0)
    for gi, (rep, conts) in enumerate(groups or [(0, [])]):   # (a job without groups gets one of 0 replicas)
        oc = []
        for kind, v in conts:
            vals = [_other(d, ci, sh) for d in range(n_keys)]
            vals[e] = None if v is None or isinstance(v, A) else v
            if isinstance(v, A):
                patches.append((ci, e, int(v)))
            oc.append((kind, vals))
            ci += 1
        for p in range(pad if gi == 0 else 0):
            oc.append((C_, [None] * n_keys))
            if wide and p == 0:
                patches.append((ci, e, WIDE_CELL))
            ci += 1
        if groups or pad:
            out.append((rep, oc))
    return (mm, out), patches


def edge_batch(mode, n_keys, sh=None, edge_keys=None, pad=0):
    """The tables of one mode as one batch.  sh: the shift of every key (None: the unnarrowable variant,
    any int64 cell and one absent WIDE_CELL per job); edge_keys: the keys that carry a table (default
    all); pad: containers without any key added to every job's first group (they enter no sum; with two
    of them every job has the two containers from which a narrowed segment saves bytes).
    -> (arrs with req as int64, cases: per job the table entry plus 'key')."""
    wide = sh is None
    shifts = [0] * n_keys if wide else list(sh)
    jobs, cases, patches, c0 = [], [], [], 0
    for e in (range(n_keys) if edge_keys is None else edge_keys):
        for case in table(shifts[e], wide):
            if case["mode"] != mode:
                continue
            job, pp = expand(case, n_keys, e, shifts, wide, pad)
            jobs.append(job)
            cases.append(dict(case, key=e))
            patches += [(c0 + c, d, v) for c, d, v in pp]
            c0 += sum(len(conts) for _, conts in job[1])
    jgo, mm, rep, gco, req, fl = WA.build(jobs, n_keys)
    for c, d, v in patches:
        assert not fl[c] >> d & 1 and req[c][d] == 0
        req[c][d] = v
    return (jgo, mm, rep, gco, np.array(req, dtype=np.int64).reshape(-1, n_keys), fl), cases


def key_shifts(n_keys, rot):
    """Different keys, different shifts: SHIFTS cycled from position rot."""
    return [SHIFTS[(rot + d) % len(SHIFTS)] for d in range(n_keys)]


def fixed_flags(fl):
    """Key-table flags (4 keys) -> the fixed-dimension call's u8: presence bits 0-3 | kind << 4."""
    fl = np.asarray(fl, np.uint32)
    return ((fl & 15) | ((fl >> KIND_SHIFT) << 4)).astype(np.uint8)


# --------------------------------------------------------------------------- the packing rule

def r16(x):
    return (x + 15) & ~15


def req_bytes(nc, nd, narrow):                 # pe_kernels.h agg_req_bytes
    return 16 + r16(nc * 4 * nd) if narrow else nc * 8 * nd


def saves_bytes(nc, nd):
    return nc > 0 and req_bytes(nc, nd, True) < req_bytes(nc, nd, False)


def key_or(cells, n_keys):
    orv = [0] * n_keys
    for row in np.asarray(cells, dtype=object).reshape(-1, n_keys).tolist():
        for d, v in enumerate(row):
            orv[d] |= int(v)
    return orv


def ctz(v):
    return (v & -v).bit_length() - 1 if v else 0


def narrowable(cells, n_keys):
    """narrow_seg's test: per key, the OR of ALL its cells (present or not) is no negative int64 and
    spans <= 32 bits above its trailing zeros."""
    return all(v < LIM and v.bit_length() - ctz(v) <= 32 for v in key_or(cells, n_keys))


def nd_of(n_keys):
    return 4 if n_keys <= 4 else 8 if n_keys <= 8 else 16


# --------------------------------------------------------------------------- the rule restated, with faults

FAULTS = {
    "not_sticky": "the flag assigned by each step, not ORed",
    "ge_hi": ">= for > at the upper limit: 2^63 - 1 counts as an overflow",
    "ge_lo": "<= for < at the lower limit: -2^63 counts as an overflow",
    "max_after_over": "the max against initmax taken after adding the overhead",
    "k_unsigned": "the replica multiplier zero-extended from 32 bits",
    "k_low31": "the replica multiplier truncated below its sign bit (k fits int32: cutting at 32 bits changes nothing)",
    "members_nowrap": "V2 members not wrapped to int32",
    "cut_after_mul": "V1: the overflow of pod x replicas judged before the min_member cut",
    "pres_from_value": "presence from value != 0 instead of the flag bit",
    "shift_plus1": "the narrowed value shifted back one bit too far",
    "shift_both_plus1": "packed and unpacked with shift + 1: the lowest mantissa bit is lost",
    "mant31": "the narrowed mantissa cut to 31 bits",
    "shift_mod32": "the shift taken modulo 32",
    "shift_key0": "key 0's shift used for every key",
}
PACK_FAULTS = ("shift_plus1", "shift_both_plus1", "mant31", "shift_mod32", "shift_key0")
V2_FAULTS = ("max_after_over", "k_unsigned", "k_low31", "members_nowrap")
V1_FAULTS = ("cut_after_mul",)


def wrap64(x):
    x &= U64
    return x - (1 << 64) if x >> 63 else x


def packed_cells(req, n_keys, fault=None):
    """Every cell through the narrowed section and back (one segment: the whole batch)."""
    orv = key_or(req, n_keys)
    shs = [ctz(v) for v in orv]
    out = []
    for row in req:
        o = []
        for d, v in enumerate(row):
            s = shs[d] + (fault == "shift_both_plus1")
            m = (int(v) >> s) & (M32 >> (fault == "mant31"))
            if fault == "shift_key0":
                s = shs[0]
            elif fault == "shift_plus1":
                s += 1
            elif fault == "shift_mod32":
                s &= 31
            o.append(wrap64(m << s))
        out.append(o)
    return out


def model(mode, jgo, mm_, rep, gco, req, fl, n_keys, fault=None, pack=False):
    """-> (values [J][n_keys] as the int64 outputs (0 where flagged), present, members (ints), flag 0 | 1,
    first [J]: the step that first left int64, or None).  Wrapped int64 arithmetic like the kernel's."""
    if pack:
        req = packed_cells(req, n_keys, fault)
    jgo, rep, gco, fl = ([int(x) for x in a] for a in (jgo, rep, gco, fl))
    J, nk = len(jgo) - 1, n_keys
    vals = np.zeros((J, nk), dtype=object)
    present, members, flag, first = [0] * J, [0] * J, [0] * J, [None] * J
    hi = LIM - 1 - (fault == "ge_hi")
    lo = -LIM + (fault == "ge_lo")
    for j in range(J):
        st = {"ovf": False, "first": None}

        def see(x, step):
            o = not lo <= x <= hi
            if o and st["first"] is None:
                st["first"] = step
            st["ovf"] = o if fault == "not_sticky" else st["ovf"] or o
            return wrap64(x)

        acc, pres, pod_cnt, mem = [0] * nk, 0, 0, 0
        mm = int(mm_[j]) if mode == V1 else 0
        for g in range(jgo[j], jgo[j + 1]):
            r = rep[g]
            if mode == V1:
                if r <= 0:
                    continue
                room = mm - pod_cnt
                if room <= 0:
                    continue
                k = min(r, room)
                pod_cnt += k
            else:
                mem += r
                k = r
                if fault == "k_unsigned":
                    k &= 0xFFFFFFFF
                elif fault == "k_low31":
                    k &= 0x7FFFFFFF
            side, initmax, main, over = [0] * nk, [0] * nk, [0] * nk, [0] * nk
            pp = 0
            for c in range(gco[g], gco[g + 1]):
                f = fl[c]
                kind = f >> KIND_SHIFT & 3
                if mode == V1 and kind != 0:
                    continue
                for d in range(nk):
                    v = int(req[c][d])
                    if not (v != 0 if fault == "pres_from_value" else f >> d & 1):
                        continue
                    pp |= 1 << d
                    if kind == C_:
                        main[d] = see(main[d] + v, "main")
                    elif kind == SIDE:
                        side[d] = see(side[d] + v, "side")
                    elif kind == OVER:
                        over[d] = see(over[d] + v, "over")
                    else:
                        initmax[d] = max(initmax[d], see(side[d] + v, "init"))
            for d in range(nk):
                if not pp >> d & 1:
                    continue
                pod = see(side[d] + main[d], "side+main")
                if fault == "max_after_over":
                    pod = max(initmax[d], see(pod + over[d], "pod+over"))
                else:
                    pod = see(max(initmax[d], pod) + over[d], "pod+over")
                if fault == "cut_after_mul":
                    see(pod * r, "mul")
                acc[d] = see(acc[d] + see(pod * k, "mul"), "acc")
            pres |= pp
        present[j] = pres
        if mode == V1:
            members[j] = pod_cnt
        else:
            members[j] = mem if fault == "members_nowrap" else ((mem + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
        flag[j] = int(st["ovf"])
        first[j] = st["first"]
        if not st["ovf"]:
            vals[j] = acc
    return vals, present, members, flag, first


def same_answers(a, b):
    """Per job: do two (values, present, members, flag, ...) answers agree?  -> bool [J]."""
    J = len(a[3])
    return np.array([list(a[0][j]) == list(b[0][j]) and int(a[1][j]) == int(b[1][j]) and int(a[2][j]) == int(b[2][j])
                     and int(a[3][j]) == int(b[3][j]) for j in range(J)], bool)


def int64_answers(checker_out):
    """WA.agg's answer as the int64 outputs: flagged jobs' values are 0."""
    vals, pres, mem, flag = checker_out
    vals = vals.copy()
    vals[np.asarray(flag) != 0] = 0
    return vals, pres, mem, (np.asarray(flag) != 0).astype(int)


def fault_applies(fault, mode, sh, others=()):
    """Can the fault show at all in a batch of this mode whose table-carrying keys lie on shifts sh (None:
    unnarrowable), beside keys of ordinary values on shifts `others`?  A V1 multiplier is positive and no
    V1 value negative; the packing faults need a narrowed section; 2^63 - 1 is on the grid of shift 0
    alone (there through V2's sums of products); shift mod 32 needs a shift of 32 or more, 31 mantissa
    bits a shift below 32, key 0's shift a key with another shift (and nonzero cells: _other)."""
    if fault in V2_FAULTS and mode != V2 or fault in V1_FAULTS and mode != V1:
        return False
    if fault in PACK_FAULTS and sh is None:
        return False
    if fault == "ge_hi":
        return sh is None or (mode == V2 and 0 in sh)
    if fault == "ge_lo":
        return mode == V2
    if fault == "shift_mod32":
        return max(sh) >= 32
    if fault == "mant31":
        return min(sh) <= 31
    if fault == "shift_key0":
        return len(set(sh) | {s for s in others if s <= 24}) > 1
    return True


# --------------------------------------------------------------------------- edge jobs among filler

SEG_BYTES = 48 * 1024
SEG_JOBS = 256


def seg_bytes(nj, ng, nc, v1, nd, fb, narrow=False):      # pe_kernels.h agg_seg_layout
    return (32 + r16((nj + 1) * 4) + (r16(nj * 4) if v1 else 0) + r16(ng * 4) + r16((ng + 1) * 4)
            + req_bytes(nc, nd, narrow) + r16(nc * fb))


class Planner:
    """The segment planner of agg_call_locked (the `plan` lambda and agg_seg_layout, read side by side)
    over ONE job range: a segment ends at seg_jobs jobs, or where it and the next job would pass SEG_BYTES
    (sizes by the wide layout).  Calls below 32768 jobs plan one range; larger ones cut the batch at
    chunk and thread edges first (PE_AGG_CHUNKS x PE_AGG_THREADS ranges), which this does not model."""

    def __init__(self, seg_jobs, v1, nd, fb):
        self.seg_jobs, self.v1, self.nd, self.fb = seg_jobs, v1, nd, fb
        self.nj = self.ng = self.nc = 0
        self.full = 0                                     # segments that ended at seg_jobs jobs

    def lane(self, ng, nc):
        """The lane the next job would get."""
        if self.nj and (self.nj == self.seg_jobs
                        or seg_bytes(self.nj + 1, self.ng + ng, self.nc + nc, self.v1, self.nd, self.fb) > SEG_BYTES):
            return 0
        return self.nj

    def add(self, ng, nc):
        ln = self.lane(ng, nc)
        if ln == 0:
            self.full += self.nj == self.seg_jobs
            self.nj = self.ng = self.nc = 0
        self.nj += 1
        self.ng += ng
        self.nc += nc
        return ln


def planned_segments(arrs, n_keys, seg_jobs, v1, fb=4):
    """How many segments the planner cuts a batch into (one job range)."""
    pl = Planner(seg_jobs, v1, nd_of(n_keys), fb)
    return sum(pl.add(g, c) == 0 for g, c in zip(*job_sizes(arrs)))


def csr_slice(arrs, a, b):
    jgo, mm, rep, gco, req, fl = arrs
    g0, g1 = int(jgo[a]), int(jgo[b])
    c0, c1 = int(gco[g0]), int(gco[g1])
    return jgo[a:b + 1] - g0, mm[a:b], rep[g0:g1], gco[g0:g1 + 1] - c0, req[c0:c1], fl[c0:c1]


def csr_concat(parts_, n_keys):
    jgo, mm, rep, gco, req, fl = [np.zeros(1, np.int32)], [], [], [np.zeros(1, np.int32)], [], []
    g_off = c_off = 0
    for p in parts_:
        jgo.append(p[0][1:] + g_off)
        mm.append(p[1])
        rep.append(p[2])
        gco.append(p[3][1:] + c_off)
        req.append(np.asarray(p[4], np.int64).reshape(-1, n_keys))
        fl.append(p[5])
        g_off += int(p[0][-1])
        c_off += int(p[3][-1])
    return (np.concatenate(jgo).astype(np.int32), np.concatenate(mm).astype(np.int32),
            np.concatenate(rep).astype(np.int32), np.concatenate(gco).astype(np.int32),
            np.concatenate(req).astype(np.int64).reshape(-1, n_keys), np.concatenate(fl).astype(np.uint32))


def job_sizes(arrs):
    jgo, gco = np.asarray(arrs[0], np.int64), np.asarray(arrs[3], np.int64)
    return np.diff(jgo).tolist(), (gco[jgo[1:]] - gco[jgo[:-1]]).tolist() if len(gco) > 1 else [0] * (len(jgo) - 1)


def assemble(edge, filler, n_keys, seg_jobs, v1, fb=4, big=None, small=None):
    """Edge jobs (a batch) placed among the filler's jobs in order, each letting filler pass until it gets
    the lane it aims at: lane 0 of a segment, the last lane (seg_jobs - 1), or, for one of them,
    directly after the oversized job `big` (a one-job batch).  Random filler jobs of wide key tables pass
    SEG_BYTES long before a segment holds 256 of them: `small` (small_filler, at least 2 seg_jobs jobs) is
    the stretch that the first job aiming at the last lane lets pass instead, so that a segment of
    seg_jobs jobs forms at every width.  -> (arrs, position of every edge job, lanes {'first': n,
    'last': n, 'after_big': n} reached, whether the plan holds a segment of seg_jobs jobs).
    The lanes are those of the key-table calls (fb 4) planned over ONE job range, as calls below 32768
    jobs are; the fixed-dimension call's u8 flags make its segments a little smaller, so where the byte
    limit ends a segment its lanes differ, and from 32768 jobs on the plan is also cut at thread and chunk
    edges that Planner does not model: there the lanes are the restatement's, not necessarily the engine's."""
    nd = nd_of(n_keys)
    pl = Planner(seg_jobs, v1, nd, fb)
    e_ng, e_nc = job_sizes(edge)
    f_ng, f_nc = job_sizes(filler)
    F, fi, pieces, pos, n_out = len(f_ng), 0, [], [], 0
    reached = {"first": 0, "last": 0, "after_big": 0}
    run0 = 0                                              # filler[run0:fi] not yet emitted

    def flush():
        nonlocal run0
        if fi > run0:
            pieces.append(csr_slice(filler, run0, fi))
        run0 = fi

    for i in range(len(e_ng)):
        aim = ("first", "last", "after_big")[i % 3]
        if aim == "after_big" and (big is None or reached["after_big"]):
            aim = "first"
        if aim == "after_big":
            flush()
            b_ng, b_nc = job_sizes(big)
            pl.add(b_ng[0], b_nc[0])
            pieces.append(big)
            n_out += 1
            want = 0
        elif aim == "last" and small is not None and not reached["last"]:
            want = seg_jobs - 1
            s_ng, s_nc = job_sizes(small)
            si = 0
            while si < len(s_ng) and pl.lane(e_ng[i], e_nc[i]) != want:
                pl.add(s_ng[si], s_nc[si])
                si += 1
            pieces.append(csr_slice(small, 0, si))
            reached[aim] += pl.add(e_ng[i], e_nc[i]) == want
            pieces.append(csr_slice(edge, i, i + 1))
            pos.append(n_out + si)
            for k in range(si, len(s_ng)):                # (the rest of the stretch follows it)
                pl.add(s_ng[k], s_nc[k])
            pieces.append(csr_slice(small, si, len(s_ng)))
            n_out += len(s_ng) + 1
            continue
        else:
            want = 0 if aim == "first" else seg_jobs - 1
            # the first job of each aim may wait for four segments' worth of filler, the others for their
            # share of what is left: they end up spread over the batch, at whatever lane that is
            wait = 4 * seg_jobs if not reached[aim] else (F - fi) // (len(e_ng) - i)
            while fi < F and wait > 0 and pl.lane(e_ng[i], e_nc[i]) != want:
                pl.add(f_ng[fi], f_nc[fi])
                fi += 1
                n_out += 1
                wait -= 1
        flush()
        reached[aim] += pl.add(e_ng[i], e_nc[i]) == want
        pieces.append(csr_slice(edge, i, i + 1))
        pos.append(n_out)
        n_out += 1
    while fi < F:
        pl.add(f_ng[fi], f_nc[fi])
        fi += 1
    flush()
    pl.add(0, 0)                                          # (closes the last segment's count)
    return csr_concat(pieces, n_keys), np.array(pos), reached, pl.full > 0 or pl.nj - 1 == seg_jobs


def _ranges(starts, lens):
    """arange(starts[i], starts[i] + lens[i]) back to back."""
    lens = np.asarray(lens, np.int64)
    ends = np.cumsum(lens)
    return np.repeat(np.asarray(starts, np.int64) - (ends - lens), lens) + np.arange(int(ends[-1]) if len(ends) else 0)


def csr_take(arrs, jobs):
    """The jobs `jobs` of a batch, in that order, as a batch."""
    jgo, mm, rep, gco, req, fl = arrs
    jgo64, gco64 = np.asarray(jgo, np.int64), np.asarray(gco, np.int64)
    ng = jgo64[jobs + 1] - jgo64[jobs]
    g = _ranges(jgo64[jobs], ng)
    nc = gco64[g + 1] - gco64[g]
    c = _ranges(gco64[g], nc)
    return (np.concatenate([[0], np.cumsum(ng)]).astype(np.int32), mm[jobs], rep[g],
            np.concatenate([[0], np.cumsum(nc)]).astype(np.int32), req[c], fl[c])


def filler_batch(J, n_keys, seed, sh=None, min_cont=0):
    """random_keys_csr filler (min_cont: only its jobs with at least so many containers).  Narrowed
    variants: every cell on its key's grid, m << sh[d] with m < 2^32; most rows keep m small enough that
    no sum leaves int64, 3 % keep all 32 bits.  The unnarrowable variant: the first container of every
    job spans more than 32 bits in key 0, so no segment that holds a container narrows."""
    if min_cont:
        arrs = random_keys_csr(2 * J + 64, n_keys, seed)
        keep = np.flatnonzero(np.asarray(job_sizes(arrs)[1]) >= min_cont)[:J]
        assert len(keep) == J
        arrs = csr_take(arrs, keep)
    else:
        arrs = random_keys_csr(J, n_keys, seed)
    return _on_grid(arrs, sh, seed + 5)


def _on_grid(arrs, sh, seed):
    jgo, mm, rep, gco, req, fl = arrs
    if sh is None:
        first = np.asarray(gco, np.int64)[jgo[:-1]]
        first = first[np.asarray(job_sizes(arrs)[1]) > 0]
        req[first, 0] |= WIDE_CELL
    else:
        rng = np.random.default_rng(seed)
        full = rng.random(len(req)) < 0.03
        for d, s in enumerate(sh):
            w = min(32, max(0, 24 - s))
            m = np.where(full, req[:, d] & M32 & ((1 << min(32, 63 - s)) - 1), req[:, d] & ((1 << w) - 1))
            req[:, d] = m << s
    return jgo, mm, rep, gco, req, fl


def small_filler(n, n_keys, seed, sh=None):
    """n filler jobs of one group each, small enough that 256 of them and an edge job stay below SEG_BYTES
    at every key width: one container per job, two for tables of up to 4 keys (from two containers on a
    narrowed segment of 4-key records saves bytes, of wider records from one).  Random values, presence
    bits, kinds, replicas and min_member like random_keys_csr's, on the batch's grids like filler_batch's."""
    nc = 2 if nd_of(n_keys) == 4 else 1
    assert saves_bytes(nc, nd_of(n_keys))
    rng = np.random.default_rng(seed)
    C = n * nc
    req = rng.integers(0, 2**40, (C, n_keys), dtype=np.int64)
    req[rng.random((C, n_keys)) < 0.3] = 0
    fl = rng.integers(0, 1 << n_keys, C, dtype=np.int64).astype(np.uint32) | (rng.integers(0, 4, C).astype(np.uint32) << KIND_SHIFT)
    rep = rng.integers(-1, 40, n).astype(np.int32)
    rep[rng.random(n) < 0.05] = RMAX
    arrs = (np.arange(n + 1, dtype=np.int32), rng.integers(-2, 60, n).astype(np.int32), rep,
            (np.arange(n + 1) * nc).astype(np.int32), req, fl)
    return _on_grid(arrs, sh, seed + 5)


def oversized_job(n_keys, sh, seed=7):
    """One job of 4 x 600 containers (more than a segment's LDS budget) on the batch's grids."""
    jgo, mm, rep, gco, _, fl8 = one_job_csr(4, 600, seed)
    rng = np.random.default_rng(seed)
    C = int(gco[-1])
    req = rng.integers(0, 1 << 20, (C, n_keys), dtype=np.int64)
    if sh is None:
        req[::7] |= WIDE_CELL
    else:
        for d, s in enumerate(sh):
            req[:, d] = (req[:, d] & ((1 << max(0, min(20, 40 - s))) - 1)) << s
    pres = rng.integers(0, 1 << n_keys, C, dtype=np.int64).astype(np.uint32)
    return jgo, mm, rep, gco, req, pres | ((fl8.astype(np.uint32) >> 4) << KIND_SHIFT)


def oversized_edge(n_keys, e, narrow, out):
    """One job whose 4096 main containers of key e sum to the largest in-range value (out: to 2^63) -- 2^63 - 1
    with cells of 2^51 and one of 2^51 - 1 (52 bits: not narrowable), or 2^63 - 2^31 on the grid of shift
    31.  -> (arrs, the exact sum)."""
    C = 4096
    req = np.zeros((C, n_keys), np.int64)
    req[:, e] = 1 << 51
    if not out:
        req[C // 3, e] -= 1 << 31 if narrow else 1
    elif not narrow:
        req[5, e] += 1                                    # 2^63 with one odd pair: still 52 bits wide
        req[6, e] -= 1
    total = int(req[:, e].astype(object).sum())
    fl = np.full(C, 1 << e, np.uint32)
    return (np.array([0, 1], np.int32), np.array([1], np.int32), np.array([1], np.int32), np.array([0, C], np.int32),
            req, fl), total
