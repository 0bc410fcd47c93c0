#!/usr/bin/env python3
"""pe_gang_capacity_tree per-call latency on the cfg5 inventory (1M nodes), in one process: median of N calls
through the C ABI after a warm-up, tables off (count given: the device selects, only the picks' answers
cross).  The hierarchy is contiguous racks (n // 245: 4096 leaves at 1M nodes) -> 128 blocks -> 4 zones -> 1
root, at J = 1 (500 calls) and for the cfg5 batch (100 000 jobs, 20 calls).  Two yardsticks on the same batch
with the same counts in the same process: pe_gang_capacity_domains with n_domains = the leaf level, and the
tree call at n_levels = 1.  Call time, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context
stream, read back from pe_last_error).  Every step runs under a watchdog of its own that ends the process
if it overruns.
    python tools/gang_capacity_tree_latency.py      (GC_NODES / GC_JOBS / GC_RACK / GC_STEP_LIMIT_S to resize)"""
import os

import numpy as np

from gang_capacity_common import JOBS, NODES, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))


def domains_call(eng, req, need, count, n_domains):
    J = req.shape[0]
    dom, slots, feas = np.zeros(J, np.int32), np.zeros(J, np.int64), np.zeros(J, np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(count), n_domains, None, None, ptr(dom), ptr(slots), ptr(feas))

    def call():
        rc = eng.lib.pe_gang_capacity_domains(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, dom, slots, feas)
    return call


def tree_call(eng, req, need, count, sizes, parent):
    J = req.shape[0]
    sizes = np.ascontiguousarray(sizes, np.int32)
    level, dom, slots = np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(J, np.int64)
    feas = np.zeros((J, len(sizes)), np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(count), None, len(sizes), ptr(sizes), ptr(parent), None, None, ptr(level),
            ptr(dom), ptr(slots), ptr(feas))

    def call():
        rc = eng.lib.pe_gang_capacity_tree(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, sizes, parent, level, dom, slots, feas)
    return call


seed = synth.SEED["cfg5"]
inv = synth.make_inventory(NODES, seed, 0.2)
req, need = synth.make_fit_jobs(JOBS, seed)
req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
count = np.ascontiguousarray(1 + (np.arange(JOBS) % 64) * 8, np.int32)          # gangs of 1 .. 505 pods
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
racks = -(-(int(island.max()) + 1) // 32) * 32          # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = [racks, blocks, zones, 1]
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)
T = sum(sizes)
print(f"levels {sizes}: the roll-up reads {12 * (T - 1)} B and writes {12 * (T - racks)} B per shape "
      f"({T - racks} upper columns over {racks} leaves = {100.0 * (T - racks) / racks:.1f} %)", flush=True)

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
for J, reps, warm, kreps in ((1, 500, 30, 100), (JOBS, 20, 3, 10)):
    with step(f"J = {J}"):
        calls = (("pe_gang_capacity_tree", tree_call(eng, req[:J], need[:J], count[:J], sizes, parent)),
                 ("pe_gang_capacity_domains", domains_call(eng, req[:J], need[:J], count[:J], racks)),
                 ("pe_gang_capacity_tree n_levels 1", tree_call(eng, req[:J], need[:J], count[:J], sizes[:1], None)))
        got = []
        for name, call in calls:
            med, p90 = bench.time_calls(call, reps, warm)
            k, _ = kernel_ms(eng, call, kreps, 2)
            got.append((med, k))
            print(f"J {J}: {name} call {med:.1f} us (p90 {p90:.1f}), kernels {k * 1e3:.1f} us", flush=True)
        # the same answers from all three where they overlap
        t, d, o = (c.keep for _, c in calls)
        assert np.array_equal(t[8][:, 0], d[5]) and np.array_equal(o[8][:, 0], d[5]) and np.array_equal(o[6], d[3])
        print(f"J {J}: tree / domains ratio call {got[0][0] / got[1][0]:.3f}, kernels {got[0][1] / got[1][1]:.3f}; "
              f"tree / one level ratio call {got[0][0] / got[2][0]:.3f}, kernels {got[0][1] / got[2][1]:.3f}; "
              f"extra per call {got[0][0] - got[1][0]:.1f} us, kernels {(got[0][1] - got[1][1]) * 1e3:.1f} us", flush=True)
eng.close()
