#!/usr/bin/env python3
"""pe_place_greedy_domains per-call latency on the cfg5 inventory (1M nodes), in one process: the cfg3 batch
(10 000 jobs), every job sent to the rack that pe_gang_capacity_tree selects for its first group (required at
rack level; a job no rack holds goes to rack j mod racks), over contiguous racks (n // 245: 4096 leaves at 1M
nodes) -> 128 blocks -> 4 zones -> 1 root.  Every job asks on the same, untouched residuals, so best fit sends
most of them to the same few racks; a second row spreads the same batch (job j to rack j mod the racks in use),
the case of an admission loop that places as it goes.  Median of N calls through the C ABI after a warm-up, with a
pe_reset_residuals between the calls (not timed); call time, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on
the context stream, read back from pe_last_error).  The yardstick is pe_place_greedy in the same process on the
same batch and inventory: its answers differ (it is not confined to racks), the pods placed are comparable,
and both are printed.  Every step runs under a watchdog of its own that ends the process if it overruns.
    python tools/place_domains_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
racks = -(-(int(island.max()) + 1) // 32) * 32          # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)

jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
P = int(cnt.sum())
pods, status = np.zeros(max(P, 1), np.int32), np.zeros(JOBS, np.int32)

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
with step("the jobs' racks"):
    first = jgo[:-1]
    tc = eng.gang_capacity_tree(req[first], need[first], np.maximum(cnt[first], 1), np.zeros(JOBS, np.int32), sizes, parent,
                                tables=False)
    selected = np.ascontiguousarray(np.where(tc.domain >= 0, tc.domain, np.arange(JOBS) % racks), np.int32)
    spread = np.ascontiguousarray(np.arange(JOBS) % (int(island.max()) + 1), np.int32)
    print(f"{JOBS} jobs, {int(jgo[-1])} groups, {P} pods; {(tc.domain >= 0).sum()} jobs have a rack for their first group",
          flush=True)
dom = selected


def domains_call():
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(dom), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def greedy_call():
    rc = eng.lib.pe_place_greedy(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def timed(call, reps, warm):
    us = []
    for i in range(warm + reps):
        eng.reset_residuals()
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            us.append((time.perf_counter() - t0) * 1e6)
    return median(us)


def placed():
    poff = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    ok = status == 0
    return int(ok.sum()), int((poff[jgo[1:]] - poff[jgo[:-1]])[ok].sum())


calls = {}
for label, dom in (("selected racks", selected), ("spread racks", spread)):
    with step(f"pe_place_greedy_domains, {label}"):
        per = np.bincount(dom, minlength=racks)
        call_us = timed(domains_call, REPS, 2)
        d_jobs, d_pods = placed()
        os.environ["PE_CAP_EVENTS"] = "1"
        ms = []
        for _ in range(REPS):
            eng.reset_residuals()
            domains_call()
            ms.append(float(re.search(r"kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode()).group(1)))
        del os.environ["PE_CAP_EVENTS"]
        calls[label] = call_us
        print(f"pe_place_greedy_domains, {label}: {(per > 0).sum()} active racks, at most {per.max()} jobs in one; call "
              f"{call_us:.0f} us, kernels {median(ms) * 1e3:.0f} us; {d_jobs} jobs placed, {d_pods} pods placed", flush=True)
with step("pe_place_greedy"):
    g_us = timed(greedy_call, REPS, 2)
    g_jobs, g_pods = placed()
    print(f"pe_place_greedy (unconstrained, the yardstick): call {g_us:.0f} us; {g_jobs} jobs placed, {g_pods} pods placed",
          flush=True)
for label, us in calls.items():
    print(f"call time ratio domains ({label}) / greedy {us / g_us:.3f}", flush=True)
eng.close()
