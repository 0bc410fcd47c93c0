"""Big-integer checker of pe_pg_min_resources_wide: the aggregation rule of CalcPGMinResources (V1,
util.go:108-145) / CoScheduling.Build (V2, coscheduling.go:103-118) restated over the CSR arrays of the
key-table call with Python ints, step for step as the kernels walk it (agg_job_t in
training-operator_amd/csrc/pe_kernels.hip), so that every intermediate can be tested against the int64
and the 128-bit range.  tests/test_wide_agg_cpu.py validates it against the C oracle
(oracle.pg_min_resources_keys) before the GPU tests rely on it for the values past int64.

Per job: flag 0 = every intermediate of every key stayed in int64 and no input was wider; 1 = some
int64 step overflowed, or some value of the job's records is >= 2^63; 2 = some intermediate left
[-2^127, 2^127) (sticky; the job's values are then 0)."""
from __future__ import annotations

import numpy as np

V1, V2 = 1, 2
KIND_SHIFT = 16
I64 = (-(1 << 63), 1 << 63)
I128 = (-(1 << 127), 1 << 127)
U64 = (1 << 64) - 1


def ints(lo, hi=None):
    """[C][nk] request limbs -> nested lists of Python ints (hi None: lo holds the values)."""
    lo = np.asarray(lo)
    vals = lo.astype(object) if lo.dtype == object else lo.astype(np.uint64).astype(object)
    if hi is not None:
        vals = vals + np.asarray(hi).astype(np.uint64).astype(object) * (1 << 64)
    return vals.tolist()


def limbs(vals):
    """Python ints (signed, 128-bit range) of any nesting -> (lo u64, hi i64) arrays, two's complement."""
    v = np.asarray(vals, dtype=object)
    lo = np.zeros(v.shape, np.uint64)
    hi = np.zeros(v.shape, np.int64)
    fl, fh = lo.reshape(-1), hi.reshape(-1)
    for i, x in enumerate(v.reshape(-1).tolist()):
        assert I128[0] <= x < I128[1], x
        fl[i] = x & U64
        fh[i] = x >> 64
    return lo, hi


class _Job:
    def __init__(self):
        self.o64 = False
        self.o128 = False

    def see(self, x):
        """Every intermediate passes through here.  Pod-level sums are unsigned in the 128-bit kernel
        (never negative: requests are not), so one range test serves both."""
        if not I64[0] <= x < I64[1]:
            self.o64 = True
        if not I128[0] <= x < I128[1]:
            self.o128 = True
        return x


def agg(mode, job_group_off, min_member, group_replicas, group_cont_off, req, cont_flags, n_keys, jobs=None):
    """-> (values [J][n_keys] Python ints (object array), present [J], members [J] int32, flag [J]) for
    the jobs in `jobs` (default all; rows of the other jobs stay 0).  req: nested lists from ints()."""
    jgo = [int(x) for x in job_group_off]
    rep = [int(x) for x in group_replicas]
    gco = [int(x) for x in group_cont_off]
    fl = [int(x) for x in cont_flags]
    J = len(jgo) - 1
    nk = n_keys
    vals = np.zeros((J, nk), dtype=object)
    present = np.zeros(J, np.uint16)
    members = np.zeros(J, np.int32)
    flag = np.zeros(J, np.uint8)
    for j in (range(J) if jobs is None else jobs):
        st = _Job()
        acc = [0] * nk
        pres = 0
        pod_cnt = 0
        mem = 0
        mm = int(min_member[j]) if mode == V1 else 0
        g0, g1 = jgo[j], jgo[j + 1]
        if g1 > g0:   # an input wider than int64 anywhere in the job's records
            for c in range(gco[g0], gco[g1]):
                if any(v >= I64[1] for v in req[c]):
                    st.o64 = True
        for g in range(g0, g1):
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
                mem = (mem + r) & 0xFFFFFFFF
                k = r
            side, initmax, main, over = [0] * nk, [0] * nk, [0] * nk, [0] * nk
            pp = 0
            for c in range(gco[g], gco[g + 1]):
                f = fl[c]
                kind = (f >> KIND_SHIFT) & 3
                if mode == V1 and kind != 0:
                    continue
                for d in range(nk):
                    if not f >> d & 1:
                        continue
                    v = req[c][d]
                    pp |= 1 << d
                    if kind == 0:
                        main[d] = st.see(main[d] + v)
                    elif kind == 2:
                        side[d] = st.see(side[d] + v)
                    elif kind == 3:
                        over[d] = st.see(over[d] + v)
                    else:
                        initmax[d] = max(initmax[d], st.see(side[d] + v))
            for d in range(nk):
                if not pp >> d & 1:
                    continue
                pod = st.see(side[d] + main[d])
                pod = max(initmax[d], pod)
                pod = st.see(pod + over[d])
                t = st.see(pod * k)
                acc[d] = st.see(acc[d] + t)
            pres |= pp
        present[j] = pres
        members[j] = pod_cnt if mode == V1 else (mem - (1 << 32) if mem >= 1 << 31 else mem)   # Go int32 wrap
        flag[j] = 2 if st.o128 else 1 if st.o64 else 0
        if not st.o128:
            for d in range(nk):
                vals[j, d] = acc[d]
    return vals, present, members, flag


# --------------------------------------------------------------------------- batches of the GPU tests
#
# Shared by tests/test_wide_agg_cpu.py (which proves with the checker that none of them holds a flag-2
# job, so "values are 0" never hides a wrong answer) and tests/test_gpu_agg_wide.py.

MIXED_J = (1, 32, 33, 257, 8192, 8193, 40000)
MIXED_KEYS = (1, 4, 5, 8, 16)
SHIFT = 22   # random_keys_csr(big=False) values are < 2^40: shifted they stay int64 inputs (< 2^62)


def job_of_container(jgo, gco):
    g_of_c = np.repeat(np.arange(len(gco) - 1), np.diff(gco))
    j_of_g = np.repeat(np.arange(len(jgo) - 1), np.diff(jgo))
    return j_of_g[g_of_c] if len(g_of_c) else np.zeros(0, np.int64)


def mixed_batch(J, n_keys, mode, every=False):
    """random_keys_csr(J, n_keys, seed, big=False) with the values of about 1 % of the jobs (at least
    one; `every`: all of them) shifted up by SHIFT bits, the first seed for which the C oracle flags at
    least one job.  -> (arrs, shifted job ids, the oracle's outputs).  The largest sum a job can reach is
    4 groups x 4 containers x 2^62 x 2^31 replicas < 2^97: no job can leave 128 bits."""
    import oracle
    from test_gpu_agg import random_keys_csr
    for seed in range(3000 + 7 * J + 13 * n_keys + mode, 10**6, 1009):
        jgo, mm, rep, gco, req, fl = random_keys_csr(J, n_keys, seed)
        rng = np.random.default_rng(seed + 2)
        picked = np.arange(J) if every else np.sort(rng.choice(J, max(1, J // 100), replace=False))
        sel = np.zeros(J, bool)
        sel[picked] = True
        req = req.copy()
        req[sel[job_of_container(jgo, gco)]] <<= SHIFT
        arrs = (jgo, mm, rep, gco, req, fl)
        want = oracle.pg_min_resources_keys(mode, *arrs)
        if want[3].any():
            return arrs, picked, want
    raise AssertionError("no seed gives an overflowing job")


def build(jobs, n_keys):
    """Hand-built jobs -> (jgo, mm, rep, gco, req as Python-int rows, flags).  jobs: [(min_member,
    [(replicas, [(kind, [value of key 0, ... | None = key absent]), ...]), ...]), ...]."""
    jgo, mm, rep, gco, req, fl = [0], [], [], [0], [], []
    for min_member, groups in jobs:
        for replicas, conts in groups:
            for kind, vals in conts:
                assert len(vals) == n_keys
                req.append([0 if v is None else v for v in vals])
                fl.append(sum(1 << d for d, v in enumerate(vals) if v is not None) | kind << KIND_SHIFT)
            rep.append(replicas)
            gco.append(len(req))
        mm.append(min_member)
        jgo.append(len(rep))
    return (np.array(jgo, np.int32), np.array(mm, np.int32), np.array(rep, np.int32), np.array(gco, np.int32), req,
            np.array(fl, np.uint32))


C_, INIT, SIDE, OVER = 0, 1, 2, 3
P = lambda e: 1 << e   # noqa: E731
RMAX = 2**31 - 1

# (name, mode, job, want values per key | None = flag 2, want flag).  Two keys: key 1 carries ordinary
# values beside key 0's wide ones (keys never interact), except where it is part of the case.
WIDE_CASES = [
    ("values up to 2^100", V2, (0, [(3, [(C_, [P(100), 7]), (C_, [P(99) + 12345, None]), (SIDE, [P(64) - 1, 1])])]),
     [3 * (P(100) + P(99) + 12345 + P(64) - 1), 24], 1),
    ("sum of exactly 2^127 - 1", V2, (0, [(1, [(C_, [P(126), 1]), (C_, [P(126) - 1, 2])])]), [P(127) - 1, 3], 1),
    ("sum of 2^127", V2, (0, [(1, [(C_, [P(126), 1]), (C_, [P(126), 2])])]), None, 2),
    ("sum of 2^127 across groups", V2, (0, [(1, [(C_, [P(126), 1])]), (1, [(C_, [P(126), 2])])]), None, 2),
    ("2^96 x (2^31 - 1) replicas", V2, (0, [(RMAX, [(C_, [P(96), 1])])]), [P(127) - P(96), RMAX], 1),
    ("2^96 x 2^31 - 1 replicas + 2^96", V2, (0, [(RMAX, [(C_, [P(96), 1])]), (1, [(C_, [P(96) - 1, 0])])]),
     [P(127) - 1, RMAX], 1),
    ("2^96 x (2^31 - 1) replicas, v1", V1, (RMAX, [(RMAX, [(C_, [P(96), 1])])]), [P(127) - P(96), RMAX], 1),
    ("(2^96 + 2^66) x (2^31 - 1) leaves 128 bits", V2, (0, [(RMAX, [(C_, [P(96) + P(66), 1])])]), None, 2),
    ("(2^96 + 2^65) x (2^31 - 1) stays", V2, (0, [(RMAX, [(C_, [P(96) + P(65), 1])])]),
     [(P(96) + P(65)) * RMAX, RMAX], 1),
    ("a product of 2^128 and more", V2, (0, [(RMAX, [(C_, [P(126), 1])])]), None, 2),
    ("replicas -1", V2, (0, [(-1, [(C_, [P(100) + 5, 3])])]), [-(P(100) + 5), -3], 1),
    ("replicas -2^31: the result -2^127", V2, (0, [(-P(31), [(C_, [P(96), None])])]), [-P(127), 0], 1),
    ("replicas -2^31 past -2^127", V2, (0, [(-P(31), [(C_, [P(96) + 1, None])])]), None, 2),
    ("-2^127 then +2^127 - 1", V2, (0, [(-P(31), [(C_, [P(96), 1])]), (1, [(C_, [P(127) - 1, 1])])]),
     [-1, 1 - P(31)], 1),
    ("lo-limb carry", V2, (0, [(1, [(C_, [P(64) - 1, 1]), (C_, [1, 1])])]), [P(64), 2], 1),
    ("lo-limb carry under the multiply", V2, (0, [(3, [(C_, [P(64) - 1, 1])])]), [3 * (P(64) - 1), 3], 1),
    ("init container larger in the hi limb only", V2,
     (0, [(2, [(SIDE, [1, 1]), (INIT, [5 * P(64), 1]), (C_, [4 * P(64) + P(64) - 10, 1])])]),
     [2 * (5 * P(64) + 1), 4], 1),
    ("main + sidecars larger than the init container", V2,
     (0, [(2, [(INIT, [5 * P(64) + 3, 1]), (SIDE, [P(64), 1]), (C_, [4 * P(64) + 4, 1])])]),
     [2 * (5 * P(64) + 4), 4], 1),
    ("overhead added after the max", V2, (0, [(1, [(INIT, [P(70), 9]), (C_, [P(69), 1]), (OVER, [P(68), 2])])]),
     [P(70) + P(68), 11], 1),
    ("v1 cut by min_member in the middle of a group", V1,
     (5, [(3, [(C_, [P(80), 1])]), (-1, [(C_, [P(120), 1])]), (5, [(C_, [P(90), 1]), (INIT, [P(126), 1])]),
          (4, [(C_, [P(126), 1])])]),
     [3 * P(80) + 2 * P(90), 5], 1),
    ("v1 sum of 2^127", V1, (9, [(2, [(C_, [P(126), 1])])]), None, 2),
    ("a wide value in a record v1 does not count", V1, (2, [(2, [(C_, [5, 1]), (INIT, [P(100), 1])])]), [10, 2], 1),
    ("one key leaves 128 bits: the whole job is 0", V2, (0, [(2, [(C_, [P(126), 5])])]), None, 2),
    ("an ordinary job between them", V2, (0, [(4, [(C_, [1000, 2]), (SIDE, [24, None])])]), [4096, 8], 0),
    ("a job without groups", V2, (0, []), [0, 0], 0),
]


def wide_case_batch(mode, with_flag2):
    """The WIDE_CASES of one mode as one batch -> (arrs with Python-int req, cases)."""
    cases = [c for c in WIDE_CASES if c[1] == mode and (with_flag2 or c[4] != 2)]
    return build([c[2] for c in cases], 2), cases


def neighbours_batch(mode):
    """An ordinary batch (values < 2^40) in which ONE job holds a wide input (hi != 0 on one present
    value): -> (arrs with int64 req, the job, req_lo, req_hi)."""
    from test_gpu_agg import random_keys_csr
    jgo, mm, rep, gco, req, fl = random_keys_csr(60, 5, 4242 + mode)
    jc = job_of_container(jgo, gco)
    c = int(np.flatnonzero((fl & 31) != 0)[10])
    d = int(np.flatnonzero([(int(fl[c]) >> k) & 1 for k in range(5)])[0])
    hi = np.zeros(req.shape, np.uint64)
    hi[c, d] = 7
    return (jgo, mm, rep, gco, req, fl), int(jc[c]), req.astype(np.uint64), hi


def oversized_batches():
    """A wide job with 4 x 600 containers and one with 9000 groups, all empty but the first (shapes of
    test_gpu_agg's oversized segments), each alone and both between ordinary jobs; 4 keys."""
    from test_gpu_agg import _concat, _one_job_csr
    from test_gpu_parity import random_csr

    def keys(a):
        jgo, mm, rep, gco, req, fl8 = a
        fl = (fl8.astype(np.uint32) & 15) | ((fl8.astype(np.uint32) >> 4) << 16)
        return jgo, mm, rep, gco, req.reshape(-1, 4), fl

    jgo, mm, rep, gco, req, fl = _one_job_csr(4, 600, 1)
    big_c = (jgo, mm, rep, gco, req << 32, fl)   # values < 2^62; 600 of them per pod pass 2^63
    jgo, mm, rep, gco, _, _ = _one_job_csr(9000, 0, 2)
    rep = rep.copy()
    rep[0] = 5
    gco = gco.copy()
    gco[1:] = 2                                  # two containers of 2^62 in the first group
    big_g = (jgo, mm, rep, gco, np.full((2, 4), 2**62, np.int64), np.full(2, 15, np.uint8))
    mid = _concat([random_csr(300, 3), big_c, random_csr(10, 4), big_g, random_csr(600, 5)])
    return [keys(big_c), keys(big_g), keys(mid)]
