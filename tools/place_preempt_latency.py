#!/usr/bin/env python3
"""pe_place_preempt_domains per-call latency on tools/place_domains_latency.py's inventory and batch (cfg5, 1M nodes in
contiguous racks of 245; the cfg3 batch of 10 000 jobs, job j sent to rack j mod the racks in use), in one process:
    (a) pe_place_greedy_domains, the yardstick
    (b) pe_place_preempt_domains with empty lists and no victims
    (c) ... on a PRE-FILLED inventory: the batch itself is placed first and its placed jobs are the victims; a second
        batch (another seed, the same racks) comes in, every job listing the victims of its rack in ascending priority,
        at most PP_LIST of them.  The share of jobs that evict is printed, not chosen
    (d) the three-call chain on (c)'s input, job by job in priority order -- pe_gang_preempt_domains for the one job,
        pe_release_gangs of the victims it names, pe_place_greedy_domains of the job, the lists cleaned of dead victims
        on the host -- over the first PP_CHAIN jobs of that order, as (c)'s own yardstick per job
Median of PD_REPS calls after 2 warm-ups; between the calls (not timed) pe_reset_residuals and, for (c) and (d),
pe_assume_gangs of the victims.  The call, and for (a) to (c) the kernels alone (PE_CAP_EVENTS=1).  Every step runs
under a watchdog of its own that ends the process if it overruns.
    python tools/place_preempt_latency.py     (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / PP_LIST / PP_CHAIN to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
LIST = int(os.environ.get("PP_LIST", "16"))
CHAIN = int(os.environ.get("PP_CHAIN", "300"))

inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
used = int(island.max()) + 1
sizes = np.ascontiguousarray([used], np.int32)
to_rack = np.ascontiguousarray(np.arange(JOBS) % used, np.int32)


def arrays(seed):
    b = synth.make_jobs(JOBS, seed, "mixed")
    return [np.ascontiguousarray(a, t) for a, t in ((b.job_group_off, np.int32), (b.priority, np.int32), (b.group_count, np.int32),
                                                    (b.group_req, np.int64), (b.group_need, np.uint32))]


jgo, pri, cnt, req, need = arrays(synth.SEED["cfg3"])
P = int(cnt.sum())
pods, status = np.zeros(max(P, 1), np.int32), np.zeros(JOBS, np.int32)
prefix, mask, empty = np.zeros(JOBS, np.int32), np.zeros(JOBS, np.uint64), np.zeros(JOBS + 1, np.int32)

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)


def greedy():
    return eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(to_rack), 0, 1,
                                           ptr(sizes), None, ptr(pods), ptr(status))


def preempt(b, V, vic, jvo, jv, out_pods, vjob):
    return lambda: eng.lib.pe_place_preempt_domains(eng.h, JOBS, *[ptr(a) for a in b], ptr(to_rack), 0, 1, ptr(sizes), None, V,
                                                    *[ptr(a) for a in vic], ptr(jvo), ptr(jv), 0, ptr(out_pods), ptr(status),
                                                    ptr(prefix), ptr(mask), ptr(vjob))


def measure(call, before=lambda: None, events=True, reps=REPS):
    """(median call us, median kernel us)."""
    us, ms = [], []
    for ev in (False, True)[:1 + events]:
        if ev:
            os.environ["PE_CAP_EVENTS"] = "1"
        for i in range(2 + reps):
            eng.reset_residuals()
            before()
            eng.synchronize()
            t0 = time.perf_counter()
            rc = call()
            dt = (time.perf_counter() - t0) * 1e6
            assert rc == 0, eng.lib.pe_last_error(eng.h)
            if i >= 2 and ev:
                ms.append(float(re.search(r"kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode()).group(1)))
            elif i >= 2:
                us.append(dt)
    os.environ.pop("PE_CAP_EVENTS", None)
    return sorted(us)[len(us) // 2], (sorted(ms)[len(ms) // 2] * 1e3 if ms else float("nan"))


rows = {}
with step("(a) pe_place_greedy_domains"):
    rows["a"] = measure(greedy)
none = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(4, np.int64), np.zeros(1, np.int32)]
with step("(b) pe_place_preempt_domains, empty lists"):
    rows["b"] = measure(preempt((jgo, pri, cnt, req, need), 0, none, empty, none[0], pods, none[0]))
# ---- the pre-filled inventory: (a)'s batch is resident, its placed jobs with a pod are the victims
eng.reset_residuals()
assert greedy() == 0
vpods = np.where(np.repeat(np.repeat(status == 0, np.diff(jgo)), cnt), pods[:P], -1).astype(np.int32)
vic = [jgo, cnt, req, vpods]
poff = np.append(0, np.cumsum(cnt))
holds = np.array([(vpods[poff[jgo[v]]:poff[jgo[v + 1]]] >= 0).any() for v in range(JOBS)])
inc = arrays(synth.SEED["cfg3"] + 1)
lists = [[] for _ in range(used)]
for v in np.argsort(pri, kind="stable"):
    if holds[v] and status[v] == 0 and len(lists[to_rack[v]]) < LIST:
        lists[to_rack[v]].append(int(v))
jvo = np.cumsum([0] + [len(lists[r]) for r in to_rack]).astype(np.int32)
jv = np.ascontiguousarray([v for r in to_rack for v in lists[r]] or [0], np.int32)
P2 = int(inc[2].sum())
pods2, vjob = np.zeros(max(P2, 1), np.int32), np.zeros(JOBS, np.int32)
resident = lambda: eng.assume_gangs(*vic)   # noqa: E731
with step("(c) pe_place_preempt_domains, pre-filled"):
    rows["c"] = measure(preempt(inc, JOBS, vic, jvo, jv, pods2, vjob), resident)
    print(f"(c) {int((status == 0).sum())} of {JOBS} jobs placed, {int((prefix > 0).sum())} of them evicted "
          f"({100 * (prefix > 0).mean():.1f} % of the batch), {int((vjob >= 0).sum())} gangs evicted", flush=True)


def chain():
    """The first CHAIN jobs of the priority order, three calls each; the victims' slots are blanked as they go."""
    left = vpods.copy()
    for j in np.argsort(-inc[1], kind="stable")[:CHAIN]:
        g0, g1 = int(inc[0][j]), int(inc[0][j + 1])
        one = [np.ascontiguousarray(a) for a in (np.array([0, g1 - g0], np.int32), inc[2][g0:g1], inc[3][g0:g1], inc[4][g0:g1])]
        live = [int(v) for v in jv[jvo[j]:jvo[j + 1]] if (left[poff[jgo[v]]:poff[jgo[v + 1]]] >= 0).any()]
        K, lst = len(live), np.ascontiguousarray(live or [0], np.int32)
        dom, m, off = to_rack[j:j + 1].copy(), np.zeros(1, np.uint64), np.array([0, K], np.int32)
        assert eng.lib.pe_gang_preempt_domains(eng.h, 1, *[ptr(a) for a in one], JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(left), 1,
                                               ptr(np.zeros(1, np.int32)), ptr(dom), ptr(off), ptr(lst), 0, 1, ptr(sizes), None,
                                               None, ptr(m), None, None) == 0
        gone = [int(lst[i]) for i in range(K) if int(m[0]) >> i & 1]
        if gone:
            named = np.full(P, -1, np.int32)
            for v in gone:
                named[poff[jgo[v]]:poff[jgo[v + 1]]] = left[poff[jgo[v]]:poff[jgo[v + 1]]]
                left[poff[jgo[v]]:poff[jgo[v + 1]]] = -1
            assert eng.lib.pe_release_gangs(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(named), None) == 0
        assert eng.lib.pe_place_greedy_domains(eng.h, 1, ptr(one[0]), ptr(np.zeros(1, np.int32)), *[ptr(a) for a in one[1:]], ptr(dom),
                                               0, 1, ptr(sizes), None, ptr(pods2), ptr(status)) == 0
    return 0


with step(f"(d) the three-call chain, {CHAIN} jobs"):
    rows["d"] = measure(chain, resident, events=False, reps=3)
for key, label in (("a", "pe_place_greedy_domains"), ("b", "pe_place_preempt_domains, empty lists"),
                   ("c", "pe_place_preempt_domains, pre-filled"), ("d", f"three-call chain, first {CHAIN} jobs")):
    print(f"({key}) {label}: call {rows[key][0]:.0f} us, kernels {rows[key][1]:.0f} us", flush=True)
print(f"(b) / (a): call {rows['b'][0] / rows['a'][0]:.3f}, kernels {rows['b'][1] / rows['a'][1]:.3f}; (c) per job "
      f"{rows['c'][0] / JOBS:.2f} us, (d) per job {rows['d'][0] / CHAIN:.1f} us", flush=True)
eng.close()
