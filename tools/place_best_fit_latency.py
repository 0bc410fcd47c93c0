#!/usr/bin/env python3
"""pe_place_best_fit_domains per-call latency on tools/first_fit_latency.py's workload, in one process: the cfg5
inventory (1M nodes) in contiguous racks of 245 under blocks, zones and a root, the cfg3 batch (10 000 jobs) and up
to FF_PAIRS candidate racks per job from pe_gang_capacity_tree's slots (every group's slots >= its count, ascending
slots of the first group), level 0.
    (a) pe_place_first_fit_domains, the yardstick on the same input
    (b) pe_place_best_fit_domains, dry run
    (c) pe_place_best_fit_domains, committed
Median of PD_REPS calls after 2 warm-ups with a pe_reset_residuals before every call (not timed): the call, and the
kernels alone with the rounds and the active racks (PE_CAP_EVENTS=1: hipEvents on the context's stream, read back from
pe_last_error); the jobs and pods placed, and the jobs the two rules place in different racks.  Printed last: (b) and
(c) over (a).  Every step runs under a watchdog of its own that ends the process if it overruns.
    python tools/place_best_fit_latency.py   (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / FF_PAIRS / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
PAIRS_PER_JOB = int(os.environ.get("FF_PAIRS", "8"))

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
G, PODS = int(jgo[-1]), int(cnt.sum())
job_pods = np.add.reduceat(cnt, jgo[:-1])
shapes, shape_of = np.unique(np.column_stack([req, need.astype(np.int64)]), axis=0, return_inverse=True)
shape_of = shape_of.reshape(-1)
s_req, s_need = np.ascontiguousarray(shapes[:, :4], np.int64), np.ascontiguousarray(shapes[:, 4], np.uint32)
tree_slots = np.zeros((len(shapes), int(sizes.sum())), np.int64)

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
with step("pe_gang_capacity_tree: the candidate pairs"):
    rc = eng.lib.pe_gang_capacity_tree(eng.h, len(shapes), ptr(s_req), ptr(s_need), None, None, len(sizes), ptr(sizes),
                                       ptr(parent), ptr(tree_slots), None, None, None, None, None)
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    rack_slots = tree_slots[:, :racks]
    ok = np.ones((JOBS, racks), dtype=bool)
    job_of = np.repeat(np.arange(JOBS), np.diff(jgo))
    for g in range(G):
        ok[job_of[g]] &= rack_slots[shape_of[g]] >= cnt[g]
    key = np.where(ok, rack_slots[shape_of[jgo[:-1]]], np.iinfo(np.int64).max)
    order = np.argsort(key, axis=1, kind="stable")[:, :PAIRS_PER_JOB]
    valid = np.take_along_axis(ok, order, axis=1)
    pair_job = np.ascontiguousarray(np.repeat(np.arange(JOBS), valid.sum(axis=1)), np.int32)
    pair_domain = np.ascontiguousarray(order[valid], np.int32)
    P = len(pair_job)
    print(f"{JOBS} jobs, {G} groups, {PODS} pods; {P} pairs on {len(np.unique(pair_domain))} racks, at most "
          f"{np.bincount(pair_domain).max()} pairs on one", flush=True)

pods, status, job_pair = np.zeros(max(PODS, 1), np.int32), np.zeros(JOBS, np.int32), np.zeros(JOBS, np.int32)
slots = np.zeros(max(P, 1), np.int64)
head = (eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job), ptr(pair_domain))
tree = (0, len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status), ptr(job_pair))
CALLS = (("a", "pe_place_first_fit_domains", lambda: eng.lib.pe_place_first_fit_domains(*head, *tree)),
         ("b", "pe_place_best_fit_domains, dry run", lambda: eng.lib.pe_place_best_fit_domains(*head, 1, *tree, ptr(slots))),
         ("c", "pe_place_best_fit_domains", lambda: eng.lib.pe_place_best_fit_domains(*head, 0, *tree, ptr(slots))))


def measure(call):
    """(median call us, median kernel us, jobs placed, pods placed, rounds of the last call, its pairs)."""
    us, ms, text = [], [], ""
    for events in (False, True):
        if events:
            os.environ["PE_CAP_EVENTS"] = "1"
        for i in range(2 + REPS):
            eng.reset_residuals()
            eng.synchronize()
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e6
            assert rc == 0, eng.lib.pe_last_error(eng.h)
            if i >= 2 and events:
                text = eng.lib.pe_last_error(eng.h).decode()
                ms.append(float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)))
            elif i >= 2:
                us.append(dt)
    del os.environ["PE_CAP_EVENTS"]
    done = status == 0
    return (sorted(us)[len(us) // 2], sorted(ms)[len(ms) // 2] * 1e3, int(done.sum()), int(job_pods[done].sum()),
            int(re.search(r"rounds=(\d+)", text).group(1)), job_pair.copy())


rows = {}
for key, label, call in CALLS:
    with step(label):
        rows[key] = r = measure(call)
        print(f"({key}) {label}: call {r[0]:.0f} us, kernels {r[1]:.0f} us, {r[4]} rounds; {r[2]} jobs placed, "
              f"{r[3]} pods placed", flush=True)
print(f"{int((rows['a'][5] != rows['c'][5]).sum())} jobs differ between first fit and best fit", flush=True)
for key in "bc":
    print(f"({key}) / (a): call {rows[key][0] / rows['a'][0]:.3f}, kernels {rows[key][1] / rows['a'][1]:.3f}, rounds "
          f"{rows[key][4] / max(rows['a'][4], 1):.3f}", flush=True)
eng.close()
