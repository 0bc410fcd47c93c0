#!/usr/bin/env python3
"""pe_place_spread_domains per-call latency on tools/place_domains_latency.py's inventory and batch (cfg5, 1M nodes in
contiguous racks of 245 -> blocks of 32 racks; the cfg3 batch of 10 000 jobs, job j sent to domain j mod the domains
in use), in one process:
    (a) pe_place_greedy_domains at rack level, the yardstick
    (b) pe_place_spread_domains with caps NULL, the same racks
    (c) ... with a cap of 1 per node, the same racks
    (d) ... with a cap of 2 per rack, every job sent to a block (level 1, spread_level 0: segments of 7840 nodes)
    (e) pe_place_greedy_domains on the same blocks, the yardstick of (d)
Median of PD_REPS calls after 2 warm-ups with a pe_reset_residuals between the calls (not timed): the call, and the
kernels alone (PE_CAP_EVENTS=1: hipEvents on the context's stream, read back from pe_last_error).  Printed: (b) / (a),
and for (c) and (d) the kernel time per decision, counting the decisions that stayed -- the runs of one node in the
pod slots of the placed jobs' groups; a failed job's decisions are rolled back and not counted.  Every step runs under
a watchdog of its own that ends the process if it overruns.
    python tools/place_spread_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))

inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
used = int(island.max()) + 1
racks = -(-used // 32) * 32
blocks = racks // 32
sizes = np.ascontiguousarray([racks, blocks, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.zeros(blocks)]), np.int32)
jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
G, P = len(cnt), int(cnt.sum())
pods, status = np.zeros(max(P, 1), np.int32), np.zeros(JOBS, np.int32)
to_rack = np.ascontiguousarray(np.arange(JOBS) % used, np.int32)
to_block = np.ascontiguousarray(np.arange(JOBS) % (-(-used // 32)), np.int32)
poff = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)


def greedy_domains(dom, level):
    return lambda: eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(dom),
                                                   level, len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))


def spread(caps, spread_level, dom, level):
    caps = None if caps is None else np.full(G, caps, np.int32)
    return lambda: eng.lib.pe_place_spread_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(caps),
                                                   spread_level, 0, ptr(dom), level, len(sizes), ptr(sizes), ptr(parent),
                                                   ptr(pods), ptr(status))


def measure(call):
    """(median call us, median kernel us, jobs placed, pods placed, decisions that stayed)."""
    us, ms = [], []
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
                ms.append(float(re.search(r"kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode()).group(1)))
            elif i >= 2:
                us.append(dt)
    del os.environ["PE_CAP_EVENTS"]
    ok = status == 0
    starts = np.zeros(P, bool)
    starts[poff[:-1][cnt > 0]] = True                      # a group's first slot starts a run
    starts[1:] |= pods[1:P] != pods[:P - 1]
    decisions = int((starts & (pods[:P] >= 0)).sum())
    return (sorted(us)[len(us) // 2], sorted(ms)[len(ms) // 2] * 1e3, int(ok.sum()),
            int((poff[jgo[1:]] - poff[jgo[:-1]])[ok].sum()), decisions)


rows = {}
for key, label, call in (("a", "pe_place_greedy_domains, racks", greedy_domains(to_rack, 0)),
                         ("b", "pe_place_spread_domains, caps NULL, racks", spread(None, -1, to_rack, 0)),
                         ("c", "pe_place_spread_domains, 1 per node, racks", spread(1, -1, to_rack, 0)),
                         ("d", "pe_place_spread_domains, 2 per rack, blocks", spread(2, 0, to_block, 1)),
                         ("e", "pe_place_greedy_domains, blocks", greedy_domains(to_block, 1))):
    with step(label):
        rows[key] = r = measure(call)
        print(f"({key}) {label}: call {r[0]:.0f} us, kernels {r[1]:.0f} us; {r[2]} jobs placed, {r[3]} pods placed, "
              f"{r[4]} decisions stayed", flush=True)
print(f"(b) / (a): call {rows['b'][0] / rows['a'][0]:.3f}, kernels {rows['b'][1] / rows['a'][1]:.3f}", flush=True)
for key in "cde":
    print(f"({key}) kernels per decision that stayed: {1e3 * rows[key][1] / max(rows[key][4], 1):.1f} ns", flush=True)
eng.close()
