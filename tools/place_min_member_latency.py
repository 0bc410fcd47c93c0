#!/usr/bin/env python3
"""pe_place_min_member_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/place_domains_latency.py's inventory, hierarchy, batch and racks: contiguous racks (n // 245: 4096 leaves at
1M nodes) -> 128 blocks -> 4 zones -> 1 root, the cfg3 batch (10 000 jobs), every job sent to the rack that
pe_gang_capacity_tree selects for its first group ("selected racks") or to rack j mod the racks in use ("spread
racks"), level 0.  Median of N calls through the C ABI after two warm-ups, an untimed pe_reset_residuals before every
call: call time, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream, read back from
pe_last_error); the jobs placed and the pods that hold a node.  Per set of racks:
    pe_place_min_member_domains at M = T           the same decisions as pe_place_greedy_domains
    pe_place_min_member_domains at M = T / 2       half of every gang mandatory, the rest as fits
    pe_place_greedy_domains                        the yardstick, on the same batch
A library named by PE_LIBRARY that predates the call runs the yardstick alone: run the tool once with the parent's
library and once with the tree's, in the same job, and compare the pe_place_greedy_domains rows.  Every step runs
under a watchdog of its own.
    python tools/place_min_member_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GC_STEP_LIMIT_S to resize)"""
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
G = int(jgo[-1])
P = int(cnt.sum())
poff = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
totals = poff[jgo[1:]] - poff[jgo[:-1]]                 # T_j
m_all = np.ascontiguousarray(totals, np.int32)
m_half = np.ascontiguousarray(totals // 2, np.int32)
pods, status = np.zeros(max(P, 1), np.int32), np.zeros(JOBS, np.int32)
group_pods, job_pods = np.zeros(max(G, 1), np.int32), np.zeros(JOBS, np.int64)

eng = Engine(0)
has_call = hasattr(eng.lib, "pe_place_min_member_domains")
print(f"library: {os.environ.get('PE_LIBRARY') or 'the tree'}; pe_place_min_member_domains: {'yes' if has_call else 'no'}",
      flush=True)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
with step("the jobs' racks"):
    first = jgo[:-1]
    tc = eng.gang_capacity_tree(req[first], need[first], np.maximum(cnt[first], 1), np.zeros(JOBS, np.int32), sizes, parent,
                                tables=False)
    selected = np.ascontiguousarray(np.where(tc.domain >= 0, tc.domain, np.arange(JOBS) % racks), np.int32)
    spread = np.ascontiguousarray(np.arange(JOBS) % (int(island.max()) + 1), np.int32)
    print(f"{JOBS} jobs, {G} groups, {P} pods; {(tc.domain >= 0).sum()} jobs have a rack for their first group", flush=True)
dom = selected
min_member = m_all


def check(rc):
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def domains_call():
    check(eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(dom), 0,
                                          len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status)))


def min_call():
    check(eng.lib.pe_place_min_member_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(min_member),
                                              ptr(dom), 0, len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status),
                                              ptr(group_pods), ptr(job_pods)))


def timed(call, reps=REPS, warm=2):
    us = []
    for i in range(warm + reps):
        eng.reset_residuals()
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            us.append((time.perf_counter() - t0) * 1e6)
    return median(us), min(us), max(us)


def kernels(call, reps=REPS):
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        ms = []
        for _ in range(reps):
            eng.reset_residuals()
            call()
            ms.append(float(re.search(r"kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode()).group(1)))
        return median(ms) * 1e3
    finally:
        del os.environ["PE_CAP_EVENTS"]


rows = {}
for label, dom in (("selected racks", selected), ("spread racks", spread)):
    per = np.bincount(dom, minlength=racks)
    todo = [("pe_place_greedy_domains", domains_call, None)]
    if has_call:
        todo += [("pe_place_min_member_domains M = T", min_call, m_all),
                 ("pe_place_min_member_domains M = T / 2", min_call, m_half)]
    for name, call, mm in todo + todo[:1]:                 # the yardstick a second time: the spread within the run
        min_member = mm
        with step(f"{name}, {label}"):
            (call_us, lo, hi), k_us = timed(call), kernels(call)
            rows.setdefault((label, name), []).append(call_us)
            print(f"{name}, {label}: {(per > 0).sum()} active racks, at most {per.max()} jobs in one; call {call_us:.0f} us "
                  f"(min {lo:.0f}, max {hi:.0f}), kernels {k_us:.0f} us; {int((status == 0).sum())} jobs placed, "
                  f"{int(job_pods.sum() if mm is not None else totals[status == 0].sum())} pods hold a node", flush=True)
for (label, name), us in rows.items():
    base = rows[label, "pe_place_greedy_domains"]
    if name != "pe_place_greedy_domains":
        print(f"call time ratio, {label}: {name} / pe_place_greedy_domains {2 * us[0] / (base[0] + base[1]):.3f} "
              f"(the yardstick's two runs: {base[0]:.0f} and {base[1]:.0f} us)", flush=True)
eng.reset_residuals()
eng.close()
