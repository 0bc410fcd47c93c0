#!/usr/bin/env python3
"""pe_gang_capacity_domains per-call latency on the cfg5 inventory (1M nodes), in one process: median of N
calls through the C ABI after a warm-up, tables off (count given: the device selects, J-sized answers
cross).  Two domain layouts of D = 4096 domains -- contiguous racks (n // ceil(N / D)) and interleaved
(n % D) -- each at J = 1 and for the cfg5 batch (100 000 jobs), with pe_gang_capacity on the same batch
in the same process as the yardstick, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context
stream, read back from pe_last_error).  Every step runs under a watchdog of its own that ends the process
if it overruns.
    python tools/gang_capacity_domains_latency.py      (GC_NODES / GC_JOBS / GC_DOMAINS / GC_STEP_LIMIT_S to resize)"""
import os

import numpy as np

from gang_capacity_common import JOBS, NODES, capacity_call, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402

DOMAINS = int(os.environ.get("GC_DOMAINS", "4096"))


def domains_call(eng, req, need, count):
    J = req.shape[0]
    dom, slots, feas = np.zeros(J, np.int32), np.zeros(J, np.int64), np.zeros(J, np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(count), DOMAINS, None, None, ptr(dom), ptr(slots), ptr(feas))

    def call():
        rc = eng.lib.pe_gang_capacity_domains(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, dom, slots, feas)
    return call


seed = synth.SEED["cfg5"]
inv = synth.make_inventory(NODES, seed, 0.2)
req, need = synth.make_fit_jobs(JOBS, seed)
req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
count = np.ascontiguousarray(1 + (np.arange(JOBS) % 64) * 8, np.int32)          # gangs of 1 .. 505 pods
ids = np.arange(NODES, dtype=np.int64)
per_rack = -(-NODES // DOMAINS)
layouts = (("contiguous racks", (ids // per_rack).astype(np.int32)), ("interleaved", (ids % DOMAINS).astype(np.int32)))

eng = Engine(0)
for name, island in layouts:
    with step(f"load {NODES} nodes, {DOMAINS} domains, {name}"):
        eng.load_nodes(inv.cap, inv.used, inv.labels, island)
    for J, reps, warm, kreps in ((1, 500, 30, 100), (JOBS, 20, 3, 10)):
        with step(f"{name}: J = {J}"):
            dom = domains_call(eng, req[:J], need[:J], count[:J])
            first, _ = bench.time_calls(dom, 1, 1)
            if first > 250e3:   # a slow layout: fewer repetitions, the step stays within its limit
                reps, warm, kreps = 5, 1, 3
            med, p90 = bench.time_calls(dom, reps, warm)
            k, _ = kernel_ms(eng, dom, kreps, 2)
            yard = capacity_call(eng, req[:J], need[:J])
            ymed, yp90 = bench.time_calls(yard, reps, warm)
            yk, _ = kernel_ms(eng, yard, kreps, 2)
            print(f"{name} J {J}: pe_gang_capacity_domains call {med:.1f} us (p90 {p90:.1f}), kernels {k * 1e3:.1f} us; "
                  f"pe_gang_capacity call {ymed:.1f} us (p90 {yp90:.1f}), kernels {yk * 1e3:.1f} us; "
                  f"ratio call {med / ymed:.2f}, kernels {k / yk:.2f}", flush=True)
eng.close()
