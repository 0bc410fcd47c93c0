#!/usr/bin/env python3
"""pe_gang_slice_tree per-call latency on the cfg5 inventory (1M nodes), in one process: median of N calls
through the C ABI after a warm-up.  Inventory, hierarchy and counts are gang_split_tree_latency.py's (racks of
n // 245 -> 128 blocks -> 4 zones -> 1 root; 1 to 1 + 63 * GS_COUNT_STEP pods), the counts rounded up to whole
slices of GL_SLICE = 8 pods, at J = 1 (500 calls) and for the cfg5 batch (100 000 jobs, 20 calls).  The slices are
asked for at node level (PE_SLICE_NODE) and at level 0.  The yardstick, on the same batch in the same process:
pe_gang_split_tree.  Call time, and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream, read back
from pe_last_error).  Under PE_LIBRARY naming a library without pe_gang_slice_tree only the yardstick is timed: that
is how the yardstick is measured on another build's library.  Every step runs under a watchdog of its own that ends
the process if it overruns.
    python tools/gang_slice_tree_latency.py      (GC_NODES / GC_JOBS / GC_RACK / GC_STEP_LIMIT_S to resize,
                                                  GS_COUNT_STEP / GS_MAX_PARTS / GL_SLICE for the gangs)"""
import os

import numpy as np

from gang_capacity_common import JOBS, NODES, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
COUNT_STEP = int(os.environ.get("GS_COUNT_STEP", "64"))
MAX_PARTS = int(os.environ.get("GS_MAX_PARTS", "16"))
SLICE = int(os.environ.get("GL_SLICE", "8"))


def split_call(eng, req, need, count, sizes, parent, max_parts, slice_level=None):
    """slice_level None: pe_gang_split_tree; else pe_gang_slice_tree with slices of SLICE pods at that level."""
    J = req.shape[0]
    level, dom, parts = np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(J, np.int32)
    pd, pp = np.zeros((J, max_parts), np.int32), np.zeros((J, max_parts), np.int32)
    spread = np.zeros((J, len(sizes)), np.int32)
    if slice_level is None:
        fn = eng.lib.pe_gang_split_tree
        args = (eng.h, J, ptr(req), ptr(need), ptr(count), None, len(sizes), ptr(sizes), ptr(parent), max_parts, ptr(level),
                ptr(dom), ptr(parts), ptr(pd), ptr(pp), ptr(spread))
        keep = ()
    else:
        fn = eng.lib.pe_gang_slice_tree
        z, sl, units = np.full(J, SLICE, np.int32), np.full(J, slice_level, np.int32), np.zeros(J, np.int64)
        args = (eng.h, J, ptr(req), ptr(need), ptr(count), ptr(z), ptr(sl), None, len(sizes), ptr(sizes), ptr(parent),
                max_parts, ptr(level), ptr(dom), ptr(units), ptr(parts), ptr(pd), ptr(pp), ptr(spread))
        keep = (z, sl, units)

    def call():
        rc = fn(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, level, dom, parts, pd, pp, spread) + keep
    return call


seed = synth.SEED["cfg5"]
inv = synth.make_inventory(NODES, seed, 0.2)
req, need = synth.make_fit_jobs(JOBS, seed)
req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
count = 1 + (np.arange(JOBS) % 64) * COUNT_STEP
count = np.ascontiguousarray(-(-count // SLICE) * SLICE, np.int32)      # whole slices
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
racks = -(-(int(island.max()) + 1) // 32) * 32
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)

eng = Engine(0)
has_slice = hasattr(eng.lib, "pe_gang_slice_tree")
print(f"levels {sizes.tolist()}, counts {int(count.min())} .. {int(count.max())}, slices of {SLICE}, max_parts {MAX_PARTS}, "
      f"pe_gang_slice_tree {'present' if has_slice else 'absent: the yardstick alone'}", flush=True)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
with step("choose the job of J = 1"):   # of the first 64 jobs (every count once) the one spread over the most leaves
    probe = split_call(eng, req[:64], need[:64], count[:64], sizes, parent, MAX_PARTS)
    probe()
    one = int(np.argmax(probe.keep[5]))
for J, reps, warm, kreps in ((1, 500, 30, 100), (JOBS, 20, 3, 10)):
    with step(f"J = {J}"):
        at = slice(one, one + 1) if J == 1 else slice(0, J)
        cnt = np.ascontiguousarray(count[at])
        calls = [("pe_gang_split_tree", split_call(eng, req[at], need[at], cnt, sizes, parent, MAX_PARTS))]
        if has_slice:
            calls.append(("pe_gang_slice_tree, node level", split_call(eng, req[at], need[at], cnt, sizes, parent, MAX_PARTS, -1)))
            calls.append(("pe_gang_slice_tree, level 0", split_call(eng, req[at], need[at], cnt, sizes, parent, MAX_PARTS, 0)))
        got = []
        for name, call in calls:
            med, p90 = bench.time_calls(call, reps, warm)
            k, _ = kernel_ms(eng, call, kreps, 2)
            got.append((med, k))
            parts = call.keep[5]
            ok = parts >= 1
            assert (call.keep[7].sum(axis=1)[ok] == cnt[ok]).all()
            print(f"J {J}: {name} call {med:.1f} us (p90 {p90:.1f}), kernels {k * 1e3:.1f} us; gangs in one leaf "
                  f"{100.0 * (parts == 1).mean():.1f} %, spread {100.0 * (parts > 1).mean():.1f} %, more than {MAX_PARTS} parts "
                  f"{100.0 * (parts < 0).mean():.1f} %, held nowhere {100.0 * (parts == 0).mean():.1f} %", flush=True)
        for (name, call), (med, k) in list(zip(calls, got))[1:]:
            os.environ["PE_CAP_EVENTS"] = "1"
            call()
            shown = eng.lib.pe_last_error(eng.h).decode()
            del os.environ["PE_CAP_EVENTS"]
            print(f"J {J}: {name} / pe_gang_split_tree ratio call {med / got[0][0]:.3f}, kernels {k / got[0][1]:.3f}; extra per "
                  f"call {med - got[0][0]:.1f} us, kernels {(k - got[0][1]) * 1e3:.1f} us ({shown.split(' kernels_ms')[0]})", flush=True)
eng.close()
