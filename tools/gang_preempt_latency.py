#!/usr/bin/env python3
"""pe_gang_preempt_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/gang_fit_latency.py's inventory and hierarchy: contiguous racks (n // 245) -> 128 blocks -> 4 zones -> 1 root.
The victims are a resident batch (the cfg3 mix under another seed) placed first with pe_place_greedy_domains, resident
job v in rack v mod CONTESTED (625 racks: 16 residents each); a resident that was not placed keeps -1 in its pod slots
and frees nothing.  The incoming batch is the cfg3 batch; every incoming job gets PAIRS_PER_JOB candidate racks among
the contested ones, and every pair the placed residents of its rack as candidate victims, in ascending priority, at
most MAX_VICTIMS of them.  Median of N calls through the C ABI after a warm-up: call time (all four outputs, and the
selection alone), and the kernels alone with the judgements made (PE_CAP_EVENTS=1, read back from pe_last_error); the
distribution of prefix and count.  The yardstick, in the same process: pe_gang_fit_domains on the same pairs, the
cost of ONE judgement per pair.  A library named by PE_LIBRARY that predates the call runs the yardstick alone, on the
same pairs.  Every step runs under a watchdog of its own.
    python tools/gang_preempt_latency.py   (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GF_PAIRS / GP_VICTIMS /
                                             GP_CONTESTED / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
PAIRS_PER_JOB = int(os.environ.get("GF_PAIRS", "8"))
MAX_VICTIMS = int(os.environ.get("GP_VICTIMS", "16"))
CONTESTED = int(os.environ.get("GP_CONTESTED", "625"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
resident = synth.make_jobs(JOBS, synth.SEED["cfg3"] + 1, "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
contested = min(CONTESTED, in_use)
racks = -(-in_use // 32) * 32
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)


def arrays(b):
    return (np.ascontiguousarray(b.job_group_off, np.int32), np.ascontiguousarray(b.priority, np.int32),
            np.ascontiguousarray(b.group_count, np.int32), np.ascontiguousarray(b.group_req, np.int64),
            np.ascontiguousarray(b.group_need, np.uint32))


jgo, pri, cnt, req, need = arrays(batch)
vgo, vpri, vcnt, vreq, vneed = arrays(resident)

eng = Engine(0)
has_call = hasattr(eng.lib, "pe_gang_preempt_domains")
print(f"library: {os.environ.get('PE_LIBRARY') or 'the tree'}; pe_gang_preempt_domains: {'yes' if has_call else 'no'}", flush=True)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
vpod, vstatus = np.full(max(int(vcnt.sum()), 1), -1, np.int32), np.zeros(JOBS, np.int32)
vrack = np.ascontiguousarray(np.arange(JOBS) % contested, np.int32)
with step("the residents: pe_place_greedy_domains"):
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(vgo), ptr(vpri), ptr(vcnt), ptr(vreq), ptr(vneed), ptr(vrack), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(vpod), ptr(vstatus))
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    placed = vstatus == 0
    print(f"{int(placed.sum())} of {JOBS} residents placed in {contested} racks, {int((vpod >= 0).sum())} pods", flush=True)
with step("the pairs and their candidate victims"):
    by_rack = [[] for _ in range(contested)]
    for v in np.argsort(vpri, kind="stable"):                              # ascending priority, ties by index
        if placed[v]:
            by_rack[v % contested].append(int(v))
    pair_job = np.ascontiguousarray(np.repeat(np.arange(JOBS), PAIRS_PER_JOB), np.int32)
    pair_domain = np.ascontiguousarray((pair_job.astype(np.int64) + 79 * np.tile(np.arange(PAIRS_PER_JOB), JOBS)) % contested, np.int32)
    P = len(pair_job)
    lists = [by_rack[d][:MAX_VICTIMS] for d in pair_domain.tolist()]
    pvo = np.ascontiguousarray(np.cumsum([0] + [len(x) for x in lists]), np.int32)
    pv = np.ascontiguousarray([v for x in lists for v in x], np.int32)
    print(f"{JOBS} incoming jobs, {P} pairs on {len(np.unique(pair_domain))} racks, {len(pv)} candidate victims listed, "
          f"at most {int(np.diff(pvo).max())} per pair", flush=True)


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


fits, first_fit = np.zeros(P, np.uint8), np.zeros(JOBS, np.int32)


def fit_call():
    rc = eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job), ptr(pair_domain),
                                     0, len(sizes), ptr(sizes), ptr(parent), ptr(fits), None, None, ptr(first_fit))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


with step("pe_gang_fit_domains on the same pairs (the yardstick: one judgement per pair)"):
    f_us = timed(fit_call, REPS, 2)
    fk_us, text = kernels_us(fit_call, REPS)
    print(f"pe_gang_fit_domains: {P} pairs, {text.split(' kernels_ms')[0]}; call {f_us:.0f} us, kernels {fk_us:.0f} us; "
          f"{fk_us / P * 1e3:.1f} ns of kernel time per judgement; pairs that fit {fits.mean():.4f}", flush=True)
if has_call:
    prefix, victims, count = np.zeros(P, np.int32), np.zeros(P, np.uint64), np.zeros(P, np.int32)
    best = np.zeros(JOBS, np.int32)

    def preempt_call(tables=True):
        rc = eng.lib.pe_gang_preempt_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), JOBS, ptr(vgo), ptr(vcnt),
                                             ptr(vreq), ptr(vpod), P, ptr(pair_job), ptr(pair_domain), ptr(pvo), ptr(pv), 0,
                                             len(sizes), ptr(sizes), ptr(parent), ptr(prefix) if tables else None,
                                             ptr(victims) if tables else None, ptr(count) if tables else None, ptr(best))
        assert rc == 0, eng.lib.pe_last_error(eng.h)

    with step("pe_gang_preempt_domains"):
        call_us = timed(preempt_call, REPS, 2)
        sel_us = timed(lambda: preempt_call(False), REPS, 2)
        k_us, text = kernels_us(preempt_call, REPS)
        judged = int(re.search(r"judged=(\d+)", text).group(1))
        print(f"pe_gang_preempt_domains: {P} pairs, {text.split(' kernels_ms')[0]}; call {call_us:.0f} us (selection only "
              f"{sel_us:.0f} us), kernels {k_us:.0f} us", flush=True)
        print(f"{judged} judgements, {judged / P:.2f} per pair; {k_us / judged * 1e3:.1f} ns of kernel time per judgement, "
              f"{k_us / judged / (fk_us / P):.2f} x the yardstick's; call time {call_us / f_us:.2f} x the fit call's", flush=True)
        assert np.array_equal(prefix == 0, fits == 1), "k = 0 is the fit call's answer"
        edges = [-1, 0, 1, 2, 3, 5, 9, 17]
        for name, a in (("prefix", prefix), ("count", count)):
            hist = ", ".join(f"{lo}{'' if hi == lo + 1 else '..' + str(hi - 1)}: {int(((a >= lo) & (a < hi)).sum())}"
                             for lo, hi in zip(edges, edges[1:] + [65]))
            print(f"{name}: {hist}", flush=True)
        print(f"fill-backs that fired: {int(((count >= 0) & (count < prefix)).sum())} pairs; jobs with an answer: "
              f"{int((best >= 0).sum())}, of them without eviction {int((count[best[best >= 0]] == 0).sum())}", flush=True)
eng.close()
