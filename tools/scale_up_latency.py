#!/usr/bin/env python3
"""pe_scale_up_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/gang_fit_latency.py's inventory, hierarchy and batch: contiguous racks (n // 245: 4096 leaves at 1M nodes) ->
128 blocks -> 4 zones -> 1 root, and the cfg3 batch (10 000 jobs).  A few thousand slots are removed first (every
SU_GAP-th node): the new slots are the first 64 of them.  The batch is placed by pe_place_greedy_domains (job j in
rack j mod SU_RACKS, few racks so that they fill up), and the pairs are every job that pe_gang_fit_domains then refuses
in its rack, with one template (a whole 8-GPU node).  Median of N calls through the C ABI after 2 warm-ups, with
pair_max 8 and 64: call time, the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream, read back from
pe_last_error with the active racks, the units and the bound of the attempts), the attempts made per pair (from
out_nodes) and the pairs answered.  The yardstick, in the same process: pe_gang_fit_domains on the same pairs -- one
attempt is one of its judgements.  Every step runs under a watchdog of its own.
    python tools/scale_up_latency.py      (GC_NODES / PD_JOBS / GC_RACK / SU_RACKS / SU_GAP / PD_REPS / GC_STEP_LIMIT_S)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
RACKS_USED = int(os.environ.get("SU_RACKS", "64"))
GAP = int(os.environ.get("SU_GAP", "251"))
GiB = 1 << 30


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
racks = -(-in_use // 32) * 32
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
with step(f"load {NODES} nodes, racks of {RACK}; remove every {GAP}th"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
    gone = np.arange(GAP - 1, NODES, GAP, dtype=np.int64)
    eng.update_nodes(gone, np.ones(len(gone), dtype=np.uint8))
    new_slot = np.ascontiguousarray(gone[:64], np.int32)
    print(f"{len(gone)} slots removed", flush=True)


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
spread = np.ascontiguousarray(np.arange(JOBS) % min(RACKS_USED, in_use), np.int32)
with step(f"pe_place_greedy_domains, {min(RACKS_USED, in_use)} racks: they fill up"):
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(spread), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    print(f"{JOBS} jobs, {S} pod slots, {int((status == 0).sum())} jobs placed", flush=True)

all_jobs = np.ascontiguousarray(np.arange(JOBS), np.int32)
a_fits = np.zeros(JOBS, np.uint8)
with step("pe_gang_fit_domains of every job in its rack: the refused ones are the pairs"):
    rc = eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), JOBS, ptr(all_jobs), ptr(spread), 0,
                                     len(sizes), ptr(sizes), ptr(parent), ptr(a_fits), None, None, None)
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    pair_job = np.ascontiguousarray(np.nonzero(a_fits == 0)[0], np.int32)
    pair_domain = np.ascontiguousarray(spread[pair_job], np.int32)
    P = len(pair_job)
    print(f"{P} pairs in {len(np.unique(pair_domain))} racks, at most {np.bincount(pair_domain).max() if P else 0} in one", flush=True)
assert P > 0, "every job fits its rack: use fewer racks (SU_RACKS)"

tmpl = np.ascontiguousarray([[96000, 768 * GiB, 8, 2048 * GiB]], np.int64)
tlab = np.ascontiguousarray([0xF], np.uint32)
pair_tmpl = np.zeros(P, np.int32)
nodes, fail = np.zeros(P, np.int32), np.zeros(P, np.int32)
o_pods, o_new, best = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(JOBS, np.int32)
f_fits, f_fail = np.zeros(P, np.uint8), np.zeros(P, np.int32)
f_pods, f_first = np.zeros(P, np.int64), np.zeros(JOBS, np.int32)


def fit_call():
    rc = eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job), ptr(pair_domain),
                                     0, len(sizes), ptr(sizes), ptr(parent), ptr(f_fits), ptr(f_fail), ptr(f_pods), ptr(f_first))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_gang_fit_domains on the same pairs (the yardstick)"):
    f_us = timed(fit_call, REPS, 2)
    fk_us, ftext = kernels_us(fit_call, REPS)
    print(f"pe_gang_fit_domains: {P} pairs, {ftext.split(' kernels_ms')[0]}; call {f_us:.0f} us, kernels {fk_us:.0f} us, "
          f"{fk_us / P * 1e3:.0f} ns of kernel per pair; pods judged per pair {f_pods.mean():.1f}", flush=True)

for K in (8, 64):
    pair_max = np.full(P, K, np.int32)

    def scale_call():
        rc = eng.lib.pe_scale_up_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), 1, ptr(tmpl), ptr(tlab),
                                         len(new_slot), ptr(new_slot), P, ptr(pair_job), ptr(pair_domain), ptr(pair_tmpl),
                                         ptr(pair_max), 0, len(sizes), ptr(sizes), ptr(parent), ptr(nodes), ptr(fail),
                                         ptr(o_pods), ptr(o_new), ptr(best))
        assert rc == 0, eng.lib.pe_last_error(eng.h)

    with step(f"pe_scale_up_domains, pair_max {K}"):
        call_us = timed(scale_call, REPS, 2)
        k_us, text = kernels_us(scale_call, REPS)
        attempts = np.where(nodes >= 0, nodes + 1, K + 1).astype(np.int64)
        print(f"pe_scale_up_domains K={K}: {P} pairs, {text.split(' kernels_ms')[0]}; call {call_us:.0f} us, kernels "
              f"{k_us:.0f} us; pairs answered {(nodes >= 0).mean():.4f}, nodes of the answered mean "
              f"{nodes[nodes >= 0].mean() if (nodes >= 0).any() else 0:.2f} max {nodes.max()}; attempts per pair "
              f"{attempts.mean():.2f}; kernel per attempt {k_us / attempts.sum() * 1e3:.0f} ns against the yardstick's "
              f"{fk_us / P * 1e3:.0f} ns per pair (ratio {k_us / attempts.sum() / (fk_us / P):.3f}); call ratio scale / fit "
              f"{call_us / f_us:.2f}", flush=True)
eng.close()
