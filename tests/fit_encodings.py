"""Plain numpy restatements of three encodings the fit kernels compare through, each with switches that make it wrong
by one rank, one digit or one bit under the shift -- the faults the threshold inventories (fit_thresholds.py) exist to
catch.  Written from the comments of pe_kernels.h, pe_lds_kernel.h and pe_engine.cpp; test code, no engine code.

  lds_fit     digit planes: node rank R = #{v <= residual} (upper bound), its digits in base B at L levels, equality
              bits scattered into one flat run of planes, threshold planes by suffix OR, per job
              [R >= c] = GE_top(c_top + 1) | (GE_top(c_top) & ( ... GE_0(c_0))), single-valued dimensions folded
              into the need planes
  i32_fit     the 32-bit compare: per dimension the shift that brings the largest request to at most INT32_MAX, valid
              only if it divides every request; residuals floor(r / 2^s) clamped to [-1, INT32_MAX]
  coded_fit   SWAR and thermometer code words: field f holds the node's rank (SWAR: plus a guard bit on top, width
              bit_length(k) + 1; thermometer: rank ones in k bits), a job its values' ranks (1-based); fit <=> no
              field borrows from its guard bit, resp. every field holds the job's bit

Every function returns [J][N] bool like fit_thresholds.fit_rows, or None where the encoding does not take the batch."""
import numpy as np

D = 4
I32MAX = (1 << 31) - 1
I64MAX = np.iinfo(np.int64).max
CODE_MAXV = 128                  # pe_kernels.h: a coded field holds fewer values than this

MUTANTS = {
    "digit": ("top_short",       # the top level with m / dv + 1 planes: GE(c_top + 1) of the largest digit reads on
              "ge_c",            # GE(c) read in place of GE(c + 1)
              "base_off",        # the single-level plane base off by one (value index 0 for rank 0)
              "rank_lower"),     # the node rank by lower bound, #{v < r}
    "i32": ("round_zero",        # the shift rounding toward zero
            "neg_zero",          # negative residuals clamped to 0
            "sat_low"),          # saturation one below INT32_MAX
    "coded": ("narrow",          # field width bit_length(k - 1) + 1
              "therm_no_minus"),  # thermometer 1 << code without the - 1
}


def _batch(req, need):
    return np.asarray(req, dtype=np.int64).reshape(-1, D), np.asarray(need, dtype=np.uint32)


# ---------------------------------------------------------------- digit planes

def plane_count(m, L, b):
    """Planes of a field of m values at L > 1 levels in base b: b at level 0, b + 1 between, m / b^(L-1) + 2 on top."""
    return (m // b ** (L - 1) + 2) + (L - 2) * (b + 1) + b


def best_base(m, L):
    """The base with the fewest planes (the smallest such)."""
    return min(range(2, m + 1), key=lambda b: (plane_count(m, L, b), b))


def lds_fit(res, labels, req, need, levels=2, base=None, mutant=None):
    """`levels` digit levels for every dimension with at least 4 distinct values (fewer: one level), base `base` or
    the one with the fewest planes."""
    res = np.asarray(res, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.uint32)
    req, need = _batch(req, need)
    N, J = res.shape[1], len(req)
    needs, need_ix = np.unique(need, return_inverse=True)
    ok = np.ones(N, dtype=bool)
    fields = []                                   # (entries [L][J], L) per digit field, planes appended to `planes`
    planes = []
    for d in range(D):
        vals, c = np.unique(req[:, d], return_inverse=True)
        m = len(vals)
        if m == 1:                                # folded into the need planes
            ok &= res[d] >= vals[0]
            continue
        R = np.searchsorted(vals, res[d], side="left" if mutant == "rank_lower" else "right")
        c = c + 1                                 # the job asks rank 1 .. m
        L = levels if m >= 4 else 1
        B = (base or best_base(m, L)) if L > 1 else m
        entries = []
        for k in range(L):
            top, dv = k == L - 1, B ** k
            dig = R // dv if top else R // dv % B
            cdig = c // dv if top else c // dv % B
            if L == 1:
                vlo, nv = (0 if mutant == "base_off" else 1), m
                cdig = c - 1                      # plane of value v (1-based) at v - 1
            else:
                vlo = 0
                nv = m // dv + (1 if mutant == "top_short" else 2) if top else (B if k == 0 else B + 1)
            P = np.zeros((nv, N), dtype=bool)
            v = dig - vlo
            keep = (v >= 0) & (v < nv)
            P[v[keep], np.flatnonzero(keep)] = True                        # equality bits
            P = np.logical_or.accumulate(P[::-1], axis=0)[::-1]            # GE(v) = E(v) | GE(v + 1)
            entries.append(sum(len(p) for p in planes) + cdig)
            planes.append(P)
        fields.append(entries)
    need_base = sum(len(p) for p in planes)
    planes.append(ok[None, :] & ((labels[None, :] & needs[:, None]) == needs[:, None]))
    flat = np.concatenate(planes)                 # one run of planes: a read past a level's last lands in the next
    fit = flat[need_base + need_ix]
    for entries in fields:
        a = flat[entries[0]]
        for e in entries[1:]:
            g = flat[e]
            h = g if mutant == "ge_c" else flat[e + 1]
            a = h | (g & a)
        fit = fit & a
    assert fit.shape == (J, N)
    return fit


# ---------------------------------------------------------------- the 32-bit compare

def i32_shifts(req):
    """Per dimension the smallest shift with (largest request >> shift) <= INT32_MAX, or None if a request of the
    batch has a bit below its dimension's shift (the int64 compare takes the batch)."""
    req = np.asarray(req, dtype=np.int64).reshape(-1, D)
    sh = []
    for d in range(D):
        s = max(0, int(req[:, d].max()).bit_length() - 31)
        if (req[:, d] & ((1 << s) - 1)).any():
            return None
        sh.append(s)
    return sh


def i32_fit(res, labels, req, need, mutant=None):
    res = np.asarray(res, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.uint32)
    req, need = _batch(req, need)
    sh = i32_shifts(req)
    if sh is None:
        return None
    fit = (labels[None, :] & need[:, None]) == need[:, None]
    for d in range(D):
        if mutant == "round_zero":
            r = np.maximum(res[d], -I64MAX)
            v = np.where(r < 0, -(-r >> sh[d]), r >> sh[d])
        else:
            v = res[d] >> sh[d]                   # arithmetic: floor(r / 2^s)
        r32 = np.clip(v, 0 if mutant == "neg_zero" else -1, I32MAX - 1 if mutant == "sat_low" else I32MAX)
        fit &= (req[:, d] >> sh[d])[:, None] <= r32[None, :]
    return fit


# ---------------------------------------------------------------- SWAR and thermometer code words

def need_chain(needs):
    """The distinct needs ordered by popcount then value, or None if they are no chain under inclusion."""
    order = sorted((int(s) for s in needs), key=lambda s: (bin(s).count("1"), s))
    if any(a & b != a for a, b in zip(order, order[1:])):
        return None
    return order


def coded_plan(ks, needs, no_therm=False, mutant=None):
    """build_codes' arithmetic.  ks: distinct values per dimension.  None: the batch is not coded (a field with
    CODE_MAXV values or more, needs that are no chain, or more than 32 bits); else (thermometer?, widths): the
    thermometer takes one bit per value of every field if those are at most 31 in all (and it is allowed), else
    field f takes bit_length(k_f) bits for the ranks 0 .. k_f and one guard bit."""
    chain = need_chain(needs)
    k5 = tuple(ks) + (len(set(int(s) for s in needs)),)
    if chain is None or any(k >= CODE_MAXV for k in k5):
        return None
    therm = not no_therm and sum(k5) <= 31
    widths = [k if therm else (k - 1 if mutant == "narrow" else k).bit_length() + 1 for k in k5]
    return (therm, widths) if sum(widths) <= 32 else None


def coded_fit(res, labels, req, need, no_therm=False, mutant=None):
    res = np.asarray(res, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.uint32)
    req, need = _batch(req, need)
    vals = [np.unique(req[:, d]) for d in range(D)]
    plan = coded_plan([len(v) for v in vals], np.unique(need), no_therm, mutant)
    if plan is None:
        return None
    therm, widths = plan
    chain = np.array(need_chain(np.unique(need)), dtype=np.uint32)
    off = np.concatenate([[0], np.cumsum(widths)[:-1]])
    # node ranks: #{v <= r} per dimension, the satisfied prefix of the chain
    ncode = [np.searchsorted(vals[d], res[d], side="right") for d in range(D)]
    sat = (labels[None, :] & chain[:, None]) == chain[:, None]
    ncode.append(np.where(sat.all(axis=0), len(chain), np.argmin(sat, axis=0)))
    jcode = [np.searchsorted(vals[d], req[:, d]) + 1 for d in range(D)]
    jcode.append(np.searchsorted(np.array([bin(s).count("1") * (1 << 33) + int(s) for s in chain]),
                                 np.array([bin(int(s)).count("1") * (1 << 33) + int(s) for s in need])) + 1)
    X = np.zeros(res.shape[1], dtype=np.uint64)
    C = np.zeros(len(req), dtype=np.uint64)
    guard = 0
    for f in range(5):
        n, j, o = ncode[f].astype(np.uint64), jcode[f].astype(np.uint64), np.uint64(off[f])
        if therm:
            fv = (np.uint64(1) << n) - np.uint64(0 if mutant == "therm_no_minus" else 1)
            C |= np.uint64(1) << (o + j - np.uint64(1))              # Y: the job's bit of the field
        else:
            g = 1 << (widths[f] - 1)
            guard |= g << int(off[f])
            fv = n | np.uint64(g)
            C |= j << o
        X |= fv << o
    M32 = np.uint64(0xFFFFFFFF)
    X &= M32
    if therm:                                    # every field holds the job's bit: (X | ~Y) == ~0
        return ((X[None, :] | (~C[:, None] & M32)) & M32) == M32
    tmp = (X[None, :] - (C[:, None] & M32)) & M32                    # every field keeps its guard bit
    return (tmp | np.uint64(~guard & 0xFFFFFFFF)) == M32


# ---------------------------------------------------------------- plane sets

def plane_set_sizes(req, need, pl_max=32):
    """build_planes' sweep for a batch of more than pl_max (field, value) pairs: jobs ordered by their selections,
    the field with the most values first; a set closes when the next job would take it past pl_max planes.  Returns
    [(planes of the set, planes the next job would have brought it to)]; the last set's second entry is None."""
    req, need = _batch(req, need)
    cols = [np.unique(req[:, d], return_inverse=True) for d in range(D)] + [np.unique(need, return_inverse=True)]
    ford = sorted(range(5), key=lambda f: -len(cols[f][0]))              # (stable, like the value counts' ties)
    pid = np.stack([cols[f][1] for f in range(5)], axis=1)
    order = sorted(range(len(req)), key=lambda j: tuple(pid[j, f] for f in ford) + (j,))
    sets, cur = [], None
    for j in order:
        mine = {(f, int(pid[j, f])) for f in range(5)}
        if cur is None or len(cur | mine) > pl_max:
            if cur is not None:
                sets.append((len(cur), len(cur | mine)))
            cur = set()
        cur |= mine
    sets.append((len(cur), None))
    return sets
