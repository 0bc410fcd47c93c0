#!/usr/bin/env python3
"""pe_drain_fit_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/gang_fit_latency.py's inventory, hierarchy and batch: contiguous racks (n // 245: 4096 leaves at 1M nodes) ->
128 blocks -> 4 zones -> 1 root, and the cfg3 batch (10 000 jobs).  The resident book is that batch as
pe_place_greedy_domains placed it (job j in rack j mod the racks in use): its arguments and its pod nodes, handed
straight back.  The candidates are every node that holds a pod, each into its own rack.  Median of N calls through the
C ABI after a warm-up: call time with and without the targets, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the
context stream, read back from pe_last_error with the active racks, the units and the evicted pods); the share of
candidates that fit.  The yardstick, in the same process: pe_gang_fit_domains on the same tree with the same number of
pairs -- pair i is job i mod the jobs in candidate i's rack.  Every step runs under a watchdog of its own.
    python tools/drain_fit_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GC_STEP_LIMIT_S to resize)"""
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
in_use = int(island.max()) + 1
racks = -(-in_use // 32) * 32                           # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)

jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
S = int(cnt.sum())

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)


def timed(call, reps, warm):
    us = []
    for i in range(warm + reps):
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            us.append((time.perf_counter() - t0) * 1e6)
    return median(us)


def kernels_us(call, reps):
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        ms = []
        for _ in range(reps):
            call()
            text = eng.lib.pe_last_error(eng.h).decode()
            ms.append(float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)))
        return median(ms) * 1e3, text
    finally:
        del os.environ["PE_CAP_EVENTS"]


pods, status = np.full(max(S, 1), -1, np.int32), np.zeros(JOBS, np.int32)
spread = np.ascontiguousarray(np.arange(JOBS) % in_use, np.int32)
with step("pe_place_greedy_domains, spread racks: the resident book"):
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(spread), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    cand_node = np.ascontiguousarray(np.unique(pods[pods >= 0]), np.int32)
    cand_domain = np.ascontiguousarray(island[cand_node], np.int32)
    C = len(cand_node)
    per_node = np.bincount(pods[pods >= 0], minlength=NODES)[cand_node]
    print(f"{JOBS} jobs, {S} pod slots, {int((status == 0).sum())} jobs placed, {int((pods >= 0).sum())} pods on {C} nodes "
          f"(at most {per_node.max()} on one) in {len(np.unique(cand_domain))} racks, at most "
          f"{np.bincount(cand_domain).max()} candidates in one", flush=True)
fits, moved = np.zeros(C, np.uint8), np.zeros(C, np.int64)
fail_slot, target = np.zeros(C, np.int64), np.zeros(max(S, 1), np.int32)


def drain_call(targets=True):
    rc = eng.lib.pe_drain_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), ptr(pods), C, ptr(cand_node),
                                      ptr(cand_domain), 0, len(sizes), ptr(sizes), ptr(parent), ptr(fits), ptr(moved),
                                      ptr(fail_slot), ptr(target) if targets else None)
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_drain_fit_domains"):
    call_us = timed(drain_call, REPS, 2)
    plain_us = timed(lambda: drain_call(False), REPS, 2)
    k_us, text = kernels_us(drain_call, REPS)
    kp_us, _ = kernels_us(lambda: drain_call(False), REPS)
    print(f"pe_drain_fit_domains: {C} candidates, {text.split(' kernels_ms')[0]}; call {call_us:.0f} us (without targets "
          f"{plain_us:.0f} us), kernels {k_us:.0f} us (without targets {kp_us:.0f} us)", flush=True)
    print(f"candidates that fit: {fits.mean():.4f} ({int((fits == 0).sum())} do not, {int(((fits == 0) & (moved > 0)).sum())} "
          f"of them after moving a pod); pods with a target {int((target[:S] >= 0).sum())} of {int(per_node.sum())}", flush=True)

# the yardstick: as many (job, rack) pairs, on the same racks -- a job that was placed in the candidate's rack
in_rack = [np.nonzero((spread == d) & (status == 0))[0] for d in range(in_use)]
pair_job = np.ascontiguousarray([in_rack[d][i % len(in_rack[d])] if len(in_rack[d]) else i % JOBS
                                 for i, d in enumerate(cand_domain)], np.int32)
f_fits, f_fail = np.zeros(C, np.uint8), np.zeros(C, np.int32)
f_pods, f_first = np.zeros(C, np.int64), np.zeros(JOBS, np.int32)


def fit_call():
    rc = eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), C, ptr(pair_job), ptr(cand_domain),
                                     0, len(sizes), ptr(sizes), ptr(parent), ptr(f_fits), ptr(f_fail), ptr(f_pods), ptr(f_first))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_gang_fit_domains, as many pairs on the same racks (the yardstick)"):
    f_us = timed(fit_call, REPS, 2)
    fk_us, ftext = kernels_us(fit_call, REPS)
    print(f"pe_gang_fit_domains: {C} pairs, {ftext.split(' kernels_ms')[0]}; call {f_us:.0f} us, kernels {fk_us:.0f} us; "
          f"pairs that fit {f_fits.mean():.4f}, pods judged per pair {f_pods.mean():.1f} against "
          f"{per_node.mean():.1f} per candidate", flush=True)
print(f"call time ratio drain / fit {call_us / f_us:.3f}, kernels {k_us / max(fk_us, 1e-9):.3f}; per candidate "
      f"{call_us / max(C, 1) * 1e3:.0f} ns", flush=True)
eng.close()
