#!/usr/bin/env python3
"""pe_gang_fit_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/place_domains_latency.py's inventory, hierarchy and batch: contiguous racks (n // 245: 4096 leaves at 1M
nodes) -> 128 blocks -> 4 zones -> 1 root, and the cfg3 batch (10 000 jobs).  The pairs are up to PAIRS_PER_JOB
candidate racks per job: a rack is a candidate when pe_gang_capacity_tree's out_tree_slots of EVERY group of the job
is >= the group's count (the necessary condition a caller can check today), candidates in ascending order of the first
group's slots (best fit).  Median of N calls through the C ABI after a warm-up: call time, and the kernels alone
(PE_CAP_EVENTS=1: hipEvents on the context stream, read back from pe_last_error with the active racks and units); the
share of pairs that fit, and the share for which the necessary condition said yes and the exact answer is no.  The
yardsticks, in the same process: the pe_gang_capacity_tree call that produced the candidates, and the "spread"
pe_place_greedy_domains call of place_domains_latency.py (job j to rack j mod the racks in use, a
pe_reset_residuals between the calls, not timed).  Every step runs under a watchdog of its own.
    python tools/gang_fit_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GF_PAIRS / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
PAIRS_PER_JOB = int(os.environ.get("GF_PAIRS", "8"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
racks = -(-in_use // 32) * 32                           # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)
T = int(sizes.sum())

jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
G = int(jgo[-1])
assert (np.diff(jgo) > 0).all(), "every job of the batch has a group"

# the distinct group shapes: one table row each
shapes, shape_of = np.unique(np.column_stack([req, need.astype(np.int64)]), axis=0, return_inverse=True)
shape_of = shape_of.reshape(-1)
s_req = np.ascontiguousarray(shapes[:, :4], np.int64)
s_need = np.ascontiguousarray(shapes[:, 4], np.uint32)
S = len(shapes)
tree_slots = np.zeros((S, T), np.int64)

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)


def tree_call():
    rc = eng.lib.pe_gang_capacity_tree(eng.h, S, ptr(s_req), ptr(s_need), None, None, len(sizes), ptr(sizes), ptr(parent),
                                       ptr(tree_slots), None, None, None, None, None)
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def timed(call, reps, warm, before=None):
    us = []
    for i in range(warm + reps):
        if before:
            before()
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            us.append((time.perf_counter() - t0) * 1e6)
    return median(us)


def kernels_us(call, reps, before=None):
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        ms = []
        for _ in range(reps):
            if before:
                before()
            call()
            text = eng.lib.pe_last_error(eng.h).decode()
            ms.append(float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)))
        return median(ms) * 1e3, text
    finally:
        del os.environ["PE_CAP_EVENTS"]


with step("pe_gang_capacity_tree: the candidates' tables"):
    tree_us = timed(tree_call, REPS, 2)
    print(f"pe_gang_capacity_tree ({S} distinct group shapes, slots table only): call {tree_us:.0f} us", flush=True)
with step("the candidate pairs"):
    rack_slots = tree_slots[:, :racks]                                     # [S][racks]
    ok = np.ones((JOBS, racks), dtype=bool)                                # every group's slots >= its count
    job_of = np.repeat(np.arange(JOBS), np.diff(jgo))
    for g in range(G):
        ok[job_of[g]] &= rack_slots[shape_of[g]] >= cnt[g]
    first = rack_slots[shape_of[jgo[:-1]]]                                 # the first group's slots, [J][racks]
    key = np.where(ok, first, np.iinfo(np.int64).max)
    order = np.argsort(key, axis=1, kind="stable")[:, :PAIRS_PER_JOB]      # ascending slots, ties to the smallest rack
    valid = np.take_along_axis(ok, order, axis=1)
    pair_job = np.ascontiguousarray(np.repeat(np.arange(JOBS), valid.sum(axis=1)), np.int32)
    pair_domain = np.ascontiguousarray(order[valid], np.int32)
    P = len(pair_job)
    print(f"{JOBS} jobs, {G} groups, {int(cnt.sum())} pods; {int(valid.any(axis=1).sum())} jobs have a candidate rack, "
          f"{P} pairs on {len(np.unique(pair_domain))} racks, at most {np.bincount(pair_domain).max()} pairs on one", flush=True)
fits, fail = np.zeros(P, np.uint8), np.zeros(P, np.int32)
n_pods, first_fit = np.zeros(P, np.int64), np.zeros(JOBS, np.int32)


def fit_call(tables=True):
    rc = eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job), ptr(pair_domain),
                                     0, len(sizes), ptr(sizes), ptr(parent), ptr(fits) if tables else None,
                                     ptr(fail) if tables else None, ptr(n_pods) if tables else None, ptr(first_fit))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_gang_fit_domains"):
    call_us = timed(fit_call, REPS, 2)
    sel_us = timed(lambda: fit_call(False), REPS, 2)
    k_us, text = kernels_us(fit_call, REPS)
    print(f"pe_gang_fit_domains: {P} pairs, {text.split(' kernels_ms')[0]}; call {call_us:.0f} us (selection only "
          f"{sel_us:.0f} us), kernels {k_us:.0f} us", flush=True)
    print(f"pairs that fit: {fits.mean():.4f}; the necessary condition said yes and the exact answer is no: "
          f"{1 - fits.mean():.4f} ({int((fits == 0).sum())} pairs, {int((first_fit < 0).sum())} jobs without a fitting "
          f"candidate, {int((fail[fits == 0] > 0).sum())} of the failing pairs past their first group)", flush=True)
pods, status = np.zeros(max(int(cnt.sum()), 1), np.int32), np.zeros(JOBS, np.int32)
spread = np.ascontiguousarray(np.arange(JOBS) % in_use, np.int32)


def place_call():
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(spread), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_place_greedy_domains, spread racks (the yardstick)"):
    p_us = timed(place_call, REPS, 2, before=eng.reset_residuals)
    pk_us, _ = kernels_us(place_call, REPS, before=eng.reset_residuals)
    eng.reset_residuals()
    print(f"pe_place_greedy_domains, spread racks: call {p_us:.0f} us, kernels {pk_us:.0f} us; {int((status == 0).sum())} "
          f"jobs placed", flush=True)
print(f"call time ratio fit / placement {call_us / p_us:.3f}, fit / tree {call_us / tree_us:.3f}; per pair "
      f"{call_us / max(P, 1) * 1e3:.0f} ns", flush=True)
eng.close()
