#!/usr/bin/env python3
"""pe_fit_explain per-call latency on the cfg5 inventory (1M nodes), in one process: median of N calls through the
C ABI after a warm-up.  Reports the call at J = 1 and for the cfg5 batch (100 000 jobs, S distinct shapes), with and
without out_near, the domain form with job j in rack j mod the racks (racks of 1600 nodes: 625 at 1M), pe_gang_capacity
on the same batch as the yardstick, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream around
the launches, read back from pe_last_error).  Every step runs under a watchdog of its own that ends the process if
it overruns.
    python tools/fit_explain_latency.py            (GC_NODES / GC_JOBS / GC_STEP_LIMIT_S to resize)"""
import numpy as np

from gang_capacity_common import JOBS, NODES, capacity_call, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402

RACK = 1600


def explain_call(eng, req, need, near, job_domain=None, level_size=None):
    req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
    J = req.shape[0]
    hist = np.zeros((J, 32), np.int64)
    nv = np.zeros((J, 4), np.uint64) if near else None
    jd = None if job_domain is None else np.ascontiguousarray(job_domain, np.int32)
    ls = None if level_size is None else np.ascontiguousarray(level_size, np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(jd), 0, 0 if ls is None else len(ls), ptr(ls), None, ptr(hist), ptr(nv))

    def call():
        rc = eng.lib.pe_fit_explain(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, hist, nv, jd, ls)
    return call


def report(what, eng, call, reps, warm):
    med, p90 = bench.time_calls(call, reps, warm)
    k, S = kernel_ms(eng, call, max(reps // 2, 5), 2)
    print(f"{what}: S {S} records, call {med:.1f} us (p90 {p90:.1f}), kernels {k * 1e3:.1f} us", flush=True)


seed = synth.SEED["cfg5"]
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
racks = int(island.max()) + 1
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng = Engine(0)
    inv = synth.make_inventory(NODES, seed, 0.2)
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
req, need = synth.make_fit_jobs(JOBS, seed)

with step("J = 1"):
    report("pe_fit_explain J 1", eng, explain_call(eng, req[:1], need[:1], True), 500, 30)
    report("pe_fit_explain J 1, no near", eng, explain_call(eng, req[:1], need[:1], False), 500, 30)
with step(f"J = {JOBS}"):
    report(f"pe_fit_explain J {JOBS}", eng, explain_call(eng, req, need, True), 20, 3)
    report(f"pe_fit_explain J {JOBS}, no near", eng, explain_call(eng, req, need, False), 20, 3)
with step(f"J = {JOBS}, job j in rack j mod {racks}"):
    jd = np.arange(JOBS) % racks
    report(f"pe_fit_explain J {JOBS}, {racks} racks", eng, explain_call(eng, req, need, True, jd, [racks]), 10, 2)
    report(f"pe_fit_explain J {JOBS}, {racks} racks, no near", eng, explain_call(eng, req, need, False, jd, [racks]), 10, 2)
with step("pe_gang_capacity, same batch (the yardstick)"):
    report(f"pe_gang_capacity J {JOBS}", eng, capacity_call(eng, req, need), 20, 3)
with step("pe_fit_explain again (run-to-run noise)"):
    report(f"pe_fit_explain J {JOBS}", eng, explain_call(eng, req, need, True), 20, 3)
eng.close()
