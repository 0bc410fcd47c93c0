#!/usr/bin/env python3
"""pe_place_skew_domains per-call latency on tools/place_domains_latency.py's inventory and batch (cfg5, 1M nodes in
contiguous racks of 245; the cfg3 batch of 10 000 jobs, job j sent to rack j mod the racks in use), in one process:
    (a) pe_place_greedy_domains, the packing yardstick
    (b) pe_place_skew_domains with every group PE_SKEW_NONE: the same answer through the new path
    (c) pe_place_skew_domains with maxSkew 1 on hostname, no book
    (d) pe_place_spread_domains with a cap of 1 per node: one pod per decision, on the jobs it can place
Median of PD_REPS calls after 2 warm-ups with a pe_reset_residuals between the calls (not timed): the call, and the
kernels alone (PE_CAP_EVENTS=1: hipEvents on the context's stream, read back from pe_last_error).  For (b) and (c) the
takes the device made (decisions=) stand against the pods placed.  Not timed here: the in-place instance (a rack of
245 fits LDS), spread domains above the node, books of existing pods.  Every step runs under a watchdog of its own
that ends the process if it overruns.
    python tools/place_skew_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GC_STEP_LIMIT_S to resize)"""
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
sizes = np.ascontiguousarray([used], np.int32)
jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
G, P = len(cnt), int(cnt.sum())
pods, status = np.zeros(max(P, 1), np.int32), np.zeros(JOBS, np.int32)
to_rack = np.ascontiguousarray(np.arange(JOBS) % used, np.int32)
one_per_node = np.full(G, 1, np.int32)
no_skew = np.full(G, -1, np.int32)
poff = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)

head = (eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need))
tail = (ptr(to_rack), 0, 1, ptr(sizes), None, ptr(pods), ptr(status))
skew = lambda v: (ptr(v), -1, None, None, None, 0)   # noqa: E731  (hostname, no book, committed)
CALLS = (("a", "pe_place_greedy_domains", lambda: eng.lib.pe_place_greedy_domains(*head, *tail)),
         ("b", "pe_place_skew_domains, all PE_SKEW_NONE", lambda: eng.lib.pe_place_skew_domains(*head, *skew(no_skew), *tail)),
         ("c", "pe_place_skew_domains, maxSkew 1 on hostname", lambda: eng.lib.pe_place_skew_domains(*head, *skew(one_per_node), *tail)),
         ("d", "pe_place_spread_domains, 1 per node", lambda: eng.lib.pe_place_spread_domains(*head, ptr(one_per_node), -1, 0, *tail)))


def measure(call):
    """(median call us, median kernel us, jobs placed, pods placed, decisions= of the last call or -1)."""
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
    ok = status == 0
    made = re.search(r"decisions=(\d+)", text)
    return (sorted(us)[len(us) // 2], sorted(ms)[len(ms) // 2] * 1e3, int(ok.sum()),
            int((poff[jgo[1:]] - poff[jgo[:-1]])[ok].sum()), int(made.group(1)) if made else -1)


rows = {}
for key, label, call in CALLS:
    with step(label):
        rows[key] = r = measure(call)
        print(f"({key}) {label}: call {r[0]:.0f} us, kernels {r[1]:.0f} us; {r[2]} jobs placed, {r[3]} pods placed"
              + (f", {r[4]} decisions, {r[3] / max(r[4], 1):.2f} pods per decision" if r[4] >= 0 else ""), flush=True)
for key, base in (("b", "a"), ("c", "a"), ("c", "d")):
    print(f"({key}) / ({base}): call {rows[key][0] / rows[base][0]:.3f}, kernels {rows[key][1] / rows[base][1]:.3f}", flush=True)
eng.close()
