#!/usr/bin/env python3
"""pe_gang_split_tree per-call latency on the cfg5 inventory (1M nodes), in one process: median of N calls
through the C ABI after a warm-up.  Inventory and hierarchy are gang_capacity_tree_latency.py's: contiguous racks
(n // 245: 4096 leaves at 1M nodes) -> 128 blocks -> 4 zones -> 1 root, at J = 1 (500 calls) and for the cfg5
batch (100 000 jobs, 20 calls).  The counts run from 1 to 1 + 63 * GS_COUNT_STEP pods, so that a share of the gangs
fits no rack and is spread over several; the share is measured and printed.  The yardstick, on the same batch in
the same process: pe_gang_capacity_tree with the selection only (out_level and out_domain, no tables).  The split is
also timed without its part rows (the numbers of parts and the spread alone cross).  Call time,
and the kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream, read back from pe_last_error).  Under
PE_LIBRARY naming a library without pe_gang_split_tree only the yardstick is timed.  Every step runs under a
watchdog of its own that ends the process if it overruns.
    python tools/gang_split_tree_latency.py      (GC_NODES / GC_JOBS / GC_RACK / GC_STEP_LIMIT_S to resize,
                                                  GS_COUNT_STEP / GS_MAX_PARTS for the gangs and the part rows)"""
import os

import numpy as np

from gang_capacity_common import JOBS, NODES, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
COUNT_STEP = int(os.environ.get("GS_COUNT_STEP", "64"))
MAX_PARTS = int(os.environ.get("GS_MAX_PARTS", "16"))


def select_call(eng, req, need, count, sizes, parent):
    J = req.shape[0]
    level, dom = np.zeros(J, np.int32), np.zeros(J, np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(count), None, len(sizes), ptr(sizes), ptr(parent), None, None, ptr(level),
            ptr(dom), None, None)

    def call():
        rc = eng.lib.pe_gang_capacity_tree(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, level, dom)
    return call


def split_call(eng, req, need, count, sizes, parent, max_parts, rows=True):
    """rows=False: the part rows are not asked for and never cross (the numbers of parts and the spread do)."""
    J = req.shape[0]
    level, dom, parts = np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(J, np.int32)
    pd, pp = (np.zeros((J, max_parts), np.int32), np.zeros((J, max_parts), np.int32)) if rows else (None, None)
    spread = np.zeros((J, len(sizes)), np.int32)
    args = (eng.h, J, ptr(req), ptr(need), ptr(count), None, len(sizes), ptr(sizes), ptr(parent), max_parts, ptr(level),
            ptr(dom), ptr(parts), ptr(pd), ptr(pp), ptr(spread))

    def call():
        rc = eng.lib.pe_gang_split_tree(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, count, level, dom, parts, pd, pp, spread)
    return call


seed = synth.SEED["cfg5"]
inv = synth.make_inventory(NODES, seed, 0.2)
req, need = synth.make_fit_jobs(JOBS, seed)
req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
count = np.ascontiguousarray(1 + (np.arange(JOBS) % 64) * COUNT_STEP, np.int32)
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
racks = -(-(int(island.max()) + 1) // 32) * 32          # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)

eng = Engine(0)
has_split = hasattr(eng.lib, "pe_gang_split_tree")
print(f"levels {sizes.tolist()}, counts 1 .. {int(count.max())}, max_parts {MAX_PARTS}, "
      f"pe_gang_split_tree {'present' if has_split else 'absent: the yardstick alone'}", flush=True)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
one = 0   # the job of J = 1: of the first 64 jobs (every count once) the one spread over the most leaves
if has_split:
    with step("choose the job of J = 1"):
        probe = split_call(eng, req[:64], need[:64], count[:64], sizes, parent, MAX_PARTS)
        probe()
        one = int(np.argmax(probe.keep[5]))
for J, reps, warm, kreps in ((1, 500, 30, 100), (JOBS, 20, 3, 10)):
    with step(f"J = {J}"):
        at = slice(one, one + 1) if J == 1 else slice(0, J)
        cnt = np.ascontiguousarray(count[at])
        calls = [("pe_gang_capacity_tree, selection only", select_call(eng, req[at], need[at], cnt, sizes, parent))]
        if has_split:
            calls.append((f"pe_gang_split_tree, max_parts {MAX_PARTS}",
                          split_call(eng, req[at], need[at], cnt, sizes, parent, MAX_PARTS)))
            calls.append(("pe_gang_split_tree, parts and spread only",
                          split_call(eng, req[at], need[at], cnt, sizes, parent, MAX_PARTS, rows=False)))
        got = []
        for name, call in calls:
            med, p90 = bench.time_calls(call, reps, warm)
            k, _ = kernel_ms(eng, call, kreps, 2)
            got.append((med, k))
            print(f"J {J}: {name} call {med:.1f} us (p90 {p90:.1f}), kernels {k * 1e3:.1f} us", flush=True)
        if has_split:
            y, s, lean = (c.keep for _, c in calls)
            assert np.array_equal(lean[5], s[5]) and np.array_equal(lean[8], s[8])
            assert np.array_equal(y[3], s[3]) and np.array_equal(y[4], s[4])          # the selection is the yardstick's
            parts = s[5]
            ok = parts >= 1
            assert (s[7].sum(axis=1)[ok] == cnt[ok]).all()
            os.environ["PE_CAP_EVENTS"] = "1"
            calls[1][1]()
            picks = int(eng.lib.pe_last_error(eng.h).decode().split("P=")[1].split()[0])
            del os.environ["PE_CAP_EVENTS"]
            print(f"J {J}: {picks} picks; gangs in one leaf {100.0 * (parts == 1).mean():.1f} %, over several "
                  f"{100.0 * (parts > 1).mean():.1f} % (mean {parts[parts > 1].mean() if (parts > 1).any() else 0:.1f} parts, "
                  f"largest {int(parts.max())}), more than {MAX_PARTS} {100.0 * (parts < 0).mean():.1f} %, held nowhere "
                  f"{100.0 * (parts == 0).mean():.1f} %", flush=True)
            print(f"J {J}: split / selection ratio call {got[1][0] / got[0][0]:.3f}, kernels {got[1][1] / got[0][1]:.3f}; "
                  f"extra per call {got[1][0] - got[0][0]:.1f} us, kernels {(got[1][1] - got[0][1]) * 1e3:.1f} us; "
                  f"extra per pick {(got[1][0] - got[0][0]) * 1e3 / picks:.1f} ns, kernels "
                  f"{(got[1][1] - got[0][1]) * 1e6 / picks:.1f} ns; without the part rows extra per call "
                  f"{got[2][0] - got[0][0]:.1f} us", flush=True)
eng.close()
