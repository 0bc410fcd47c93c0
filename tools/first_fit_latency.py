#!/usr/bin/env python3
"""pe_place_first_fit_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/gang_fit_latency.py's inventory, hierarchy, batch and candidates: contiguous racks (n // 245: 4096 leaves at
1M nodes) -> 128 blocks -> 4 zones -> 1 root, the cfg3 batch (10 000 jobs), and up to FF_PAIRS candidate racks per
job from pe_gang_capacity_tree's slots (every group's slots >= its count, ascending slots of the first group), level
0.  Median of N calls through the C ABI after two warm-ups, an untimed pe_reset_residuals before every call: call
time, and the kernels alone with the rounds and the active racks (PE_CAP_EVENTS=1, read back from pe_last_error);
the jobs and pods placed.  The yardsticks, the same way:
    pe_gang_fit_domains (out_first only) followed by pe_place_greedy_domains on those choices -- what a caller does
        for a batch without this call; NOT the same answer: every job selects on the untouched residuals
    pe_place_greedy, unconstrained
A library named by PE_LIBRARY that predates the call runs the yardsticks alone.  Every step runs under a watchdog of
its own.
    python tools/first_fit_latency.py      (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / FF_PAIRS / GC_STEP_LIMIT_S to resize;
                                            FF_YARDSTICKS=0: the new call alone)"""
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


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
racks = -(-in_use // 32) * 32                           # whole blocks: 4082 racks in use -> a level of 4096
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)
T = int(sizes.sum())

jgo = np.ascontiguousarray(batch.job_group_off, np.int32)
pri = np.ascontiguousarray(batch.priority, np.int32)
cnt = np.ascontiguousarray(batch.group_count, np.int32)
req = np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
G = int(jgo[-1])
PODS = int(cnt.sum())
job_pods = np.add.reduceat(cnt, jgo[:-1])
assert (np.diff(jgo) > 0).all(), "every job of the batch has a group"

shapes, shape_of = np.unique(np.column_stack([req, need.astype(np.int64)]), axis=0, return_inverse=True)
shape_of = shape_of.reshape(-1)
s_req = np.ascontiguousarray(shapes[:, :4], np.int64)
s_need = np.ascontiguousarray(shapes[:, 4], np.uint32)
S = len(shapes)
tree_slots = np.zeros((S, T), np.int64)

eng = Engine(0)
has_call = hasattr(eng.lib, "pe_place_first_fit_domains")
print(f"library: {os.environ.get('PE_LIBRARY') or 'the tree'}; pe_place_first_fit_domains: {'yes' if has_call else 'no'}", flush=True)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)


def check(rc):
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def timed(call, reps=REPS, warm=2):
    us = []
    for i in range(warm + reps):
        eng.reset_residuals()
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            us.append((time.perf_counter() - t0) * 1e6)
    return median(us)


def kernels(call, reps=REPS):
    """(median kernel time in us of `reps` calls, the last call's report) for a call that makes one engine call."""
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        ms = []
        for _ in range(reps):
            eng.reset_residuals()
            call()
            text = eng.lib.pe_last_error(eng.h).decode()
            ms.append(float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)))
        return median(ms) * 1e3, text.split(" kernels_ms")[0]
    finally:
        del os.environ["PE_CAP_EVENTS"]


with step("pe_gang_capacity_tree: the candidate pairs"):
    check(eng.lib.pe_gang_capacity_tree(eng.h, S, ptr(s_req), ptr(s_need), None, None, len(sizes), ptr(sizes), ptr(parent),
                                        ptr(tree_slots), None, None, None, None, None))
    rack_slots = tree_slots[:, :racks]                                     # [S][racks]
    ok = np.ones((JOBS, racks), dtype=bool)                                # every group's slots >= its count
    job_of = np.repeat(np.arange(JOBS), np.diff(jgo))
    for g in range(G):
        ok[job_of[g]] &= rack_slots[shape_of[g]] >= cnt[g]
    first = rack_slots[shape_of[jgo[:-1]]]                                 # the first group's slots, [J][racks]
    key = np.where(ok, first, np.iinfo(np.int64).max)
    order = np.argsort(key, axis=1, kind="stable")[:, :PAIRS_PER_JOB]      # ascending slots, ties to the smallest rack
    valid = np.take_along_axis(ok, order, axis=1)
    pair_job = np.ascontiguousarray(np.repeat(np.arange(JOBS), valid.sum(axis=1)), np.int32)
    pair_domain = np.ascontiguousarray(order[valid], np.int32)
    P = len(pair_job)
    print(f"{JOBS} jobs, {G} groups, {PODS} pods; {int(valid.any(axis=1).sum())} jobs have a candidate rack, "
          f"{P} pairs on {len(np.unique(pair_domain))} racks, at most {np.bincount(pair_domain).max()} pairs on one", flush=True)

pods, status = np.zeros(max(PODS, 1), np.int32), np.zeros(JOBS, np.int32)
job_pair, first_fit = np.zeros(JOBS, np.int32), np.zeros(JOBS, np.int32)


def placed():
    return f"{int((status == 0).sum())} jobs and {int(job_pods[status == 0].sum())} pods placed"


if has_call:
    def first_fit_call():
        check(eng.lib.pe_place_first_fit_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job),
                                                 ptr(pair_domain), 0, len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status),
                                                 ptr(job_pair)))

    with step("pe_place_first_fit_domains"):
        call_us = timed(first_fit_call)
        k_us, text = kernels(first_fit_call)
        print(f"pe_place_first_fit_domains: {P} pairs, {text}; call {call_us:.0f} us, kernels {k_us:.0f} us; {placed()}; "
              f"{int(((job_pair >= 0) & (job_pair != np.searchsorted(pair_job, np.arange(JOBS)))).sum())} jobs placed by a "
              f"pair that is not their first", flush=True)


def fit_call():
    check(eng.lib.pe_gang_fit_domains(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), P, ptr(pair_job), ptr(pair_domain),
                                      0, len(sizes), ptr(sizes), ptr(parent), None, None, None, ptr(first_fit)))


# the jobs out_first chose a rack for, as a batch of their own
chosen = {}


def place_chosen():
    c = chosen
    check(eng.lib.pe_place_greedy_domains(eng.h, len(c["jobs"]), ptr(c["jgo"]), ptr(c["pri"]), ptr(c["cnt"]), ptr(c["req"]),
                                          ptr(c["need"]), ptr(c["dom"]), 0, len(sizes), ptr(sizes), ptr(parent), ptr(c["pods"]),
                                          ptr(c["status"])))


def choose():
    """The jobs out_first chose a rack for, as a batch of their own (the same at every repetition: untimed)."""
    eng.reset_residuals()
    fit_call()
    jobs = np.nonzero(first_fit >= 0)[0]
    groups = np.concatenate([np.arange(jgo[j], jgo[j + 1]) for j in jobs]) if len(jobs) else np.zeros(0, np.int64)
    chosen.update(jobs=jobs, jgo=np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.diff(jgo)[jobs])]), np.int32),
                  pri=np.ascontiguousarray(pri[jobs]), cnt=np.ascontiguousarray(cnt[groups]), req=np.ascontiguousarray(req[groups]),
                  need=np.ascontiguousarray(need[groups]), dom=np.ascontiguousarray(pair_domain[first_fit[jobs]], np.int32),
                  pods=np.zeros(max(int(cnt[groups].sum()), 1), np.int32), status=np.zeros(max(len(jobs), 1), np.int32))


def select_then_place():
    fit_call()
    place_chosen()


if os.environ.get("FF_YARDSTICKS", "1") == "0":
    eng.close()
    raise SystemExit(0)
with step("pe_gang_fit_domains (out_first), then pe_place_greedy_domains on those choices"):
    choose()
    both_us = timed(select_then_place)
    fit_us = timed(fit_call)
    pk_us, text = kernels(place_chosen)
    st = chosen["status"][:len(chosen["jobs"])]
    done = chosen["jobs"][st == 0]
    print(f"select, then place: call {both_us:.0f} us (the selection alone {fit_us:.0f} us; the placement's kernels "
          f"{pk_us:.0f} us, {text}); {len(chosen['jobs'])} jobs selected a rack, {len(done)} jobs and "
          f"{int(job_pods[done].sum())} pods placed", flush=True)


def greedy_call():
    check(eng.lib.pe_place_greedy(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(pods), ptr(status)))


with step("pe_place_greedy, unconstrained"):
    g_us = timed(greedy_call, reps=min(REPS, 3), warm=1)
    print(f"pe_place_greedy: call {g_us:.0f} us; {placed()}", flush=True)
eng.reset_residuals()
if has_call:
    print(f"call time ratio first fit / (select, then place) {call_us / both_us:.3f}, first fit / greedy {call_us / g_us:.3f}; "
          f"per pair {call_us / max(P, 1) * 1e3:.0f} ns", flush=True)
eng.close()
