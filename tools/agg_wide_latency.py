#!/usr/bin/env python3
"""pe_pg_min_resources_wide per-call latency beside pe_pg_min_resources_keys on the same batch, in one
process: median of N calls through the C ABI (ctypes pointers built once).  The bench's v1 batch as a
4-key table; "wide" rows shift the values of 1 % of the jobs (the one job at J = 1) so that their
sums leave int64 and the 128-bit kernel answers them.  The keys call is timed twice (before and
after the wide call): the difference between its two medians is the run-to-run noise.
    python tools/agg_wide_latency.py"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "training-operator_amd")]
import bench  # noqa: E402
from placement import V1, Engine, synth  # noqa: E402

P = ctypes.c_void_p


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


def calls(eng, arrs):
    jgo, mm, rep, gco, req, fl = [np.ascontiguousarray(a) for a in arrs]
    J, nk = len(jgo) - 1, req.shape[1]
    res, hi = np.zeros((J, nk), np.int64), np.zeros((J, nk), np.int64)
    pres, mem, ovf = np.zeros(J, np.uint16), np.zeros(J, np.int32), np.zeros(J, np.uint8)
    keep = (jgo, mm, rep, gco, req, fl, res, hi, pres, mem, ovf)
    k_args = (eng.h, V1, J, nk, ptr(jgo), ptr(mm), ptr(rep), ptr(gco), ptr(req), ptr(fl), ptr(res), ptr(pres),
              ptr(mem), ptr(ovf))
    w_args = (eng.h, V1, J, nk, ptr(jgo), ptr(mm), ptr(rep), ptr(gco), ptr(req), None, ptr(fl), ptr(res), ptr(hi),
              ptr(pres), ptr(mem), ptr(ovf))

    def keys():
        return eng.lib.pe_pg_min_resources_keys(*k_args)

    def wide():
        return eng.lib.pe_pg_min_resources_wide(*w_args)
    keys.keep = wide.keep = keep
    return keys, wide, ovf


eng = Engine(0)
sizes = [int(x) for x in os.environ.get("AGG_WIDE_SIZES", "1,100000").split(",")]
jgo, mm, rep, gco, req, fl8 = synth.make_pg_batch(max(sizes), synth.SEED["cfg3"])
fl = (fl8.astype(np.uint32) & 15) | ((fl8.astype(np.uint32) >> 4) << 16)
for J in sizes:
    sub = list(bench.pg_slice((jgo, mm, rep, gco, req.reshape(-1, 4), fl), 0, J))
    n, warm = (2000, 50) if J <= 1024 else (40, 5)
    keys, wide, ovf = calls(eng, sub)
    k1, _ = bench.time_calls(keys, n, warm)
    w0, _ = bench.time_calls(wide, n, warm)
    k2, _ = bench.time_calls(keys, n, warm)
    assert not ovf.any()
    # 1 % of the jobs (at least one) wide: their values scaled up to just below 2^62
    big = [a.copy() for a in sub]
    jc = np.repeat(np.repeat(np.arange(J), np.diff(big[0])), np.diff(big[3]))
    sel = np.zeros(J, bool)
    sel[::100] = True
    rows = sel[jc]
    big[4][rows] = np.where(big[4][rows] > 0, (1 << 61) + big[4][rows], 0)
    big[2][:] = np.maximum(big[2], 4)
    big[1][:] = np.maximum(big[1], 4)
    _, wide_b, ovf_b = calls(eng, big)
    before = eng.stats()["agg_wide_jobs"]
    assert wide_b() == 0
    n_wide = eng.stats()["agg_wide_jobs"] - before
    w1, _ = bench.time_calls(wide_b, n, warm)
    print(f"J {J}: keys {k1:.1f} / {k2:.1f} us, wide call without a wide job {w0:.1f} us, "
          f"with {n_wide} wide jobs {w1:.1f} us", flush=True)
eng.close()
