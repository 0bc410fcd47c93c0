#!/usr/bin/env python3
"""pe_release_gangs / pe_assume_gangs per-call latency on the cfg5 inventory (1M nodes, racks of 245), in one process,
with tools/gang_preempt_latency.py's inventory and hierarchy.  The gangs are the cfg3 batch placed with
pe_place_greedy_domains, job j in rack j mod CONTESTED.  Measured: the release and the assume of that whole placement
and of one gang, median of N calls through the C ABI after a warm-up, the opposite call restoring the state between
two measured ones; the kernel alone and the host plan (PE_CAP_EVENTS=1, read back from pe_last_error).  The yardstick,
in the same process: the workaround the calls replace -- pe_update_nodes with PE_NODE_SET of the same touched nodes
and recomputed cap / used (which also overwrites the reset snapshot of those nodes).  Every step runs under a watchdog
of its own.
    python tools/gang_ledger_latency.py   (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / GP_CONTESTED / GC_STEP_LIMIT_S to
                                           resize)"""
import ctypes
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
CONTESTED = int(os.environ.get("GP_CONTESTED", "625"))
WARM = 2


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
contested = min(CONTESTED, in_use)
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

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
pods, status = np.full(max(int(cnt.sum()), 1), -1, np.int32), np.zeros(JOBS, np.int32)
rack = np.ascontiguousarray(np.arange(JOBS) % contested, np.int32)
with step("the placement: pe_place_greedy_domains"):
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(rack), 0, len(sizes),
                                         ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    after = eng.read_residuals()
    touched = np.unique(pods[pods >= 0]).astype(np.int64)
    print(f"{int((status == 0).sum())} of {JOBS} jobs placed in {contested} racks, {int((pods >= 0).sum())} pods on "
          f"{len(touched)} nodes", flush=True)

# one gang: the placed job with the most pods
poff = np.concatenate([[0], np.cumsum(cnt)])
job_pods = poff[jgo[1:]] - poff[jgo[:-1]]
one = int(np.argmax(np.where(status == 0, job_pods, -1)))
g0, g1 = int(jgo[one]), int(jgo[one + 1])
one_off = np.ascontiguousarray([0, g1 - g0], np.int32)
one_cnt, one_req = np.ascontiguousarray(cnt[g0:g1]), np.ascontiguousarray(req[g0:g1])
one_pods = np.ascontiguousarray(pods[poff[g0]:poff[g1]])
one_touched = np.unique(one_pods[one_pods >= 0]).astype(np.int64)
WHOLE = (JOBS, jgo, cnt, req, pods)
ONE = (1, one_off, one_cnt, one_req, one_pods)
counted = ctypes.c_int64()


def ledger(fn, gangs):
    n, off, c, q, p = gangs
    rc = getattr(eng.lib, fn)(eng.h, n, ptr(off), ptr(c), ptr(q), ptr(p), ctypes.byref(counted))
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def timed(call, restore):
    """Median call time in us; `restore` (untimed) puts the state back after every call."""
    us = []
    for i in range(WARM + REPS):
        eng.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= WARM:
            us.append((time.perf_counter() - t0) * 1e6)
        restore()
    return median(us)


def inside(call, restore):
    """(median kernel us, median plan us, the last call's note) with PE_CAP_EVENTS=1."""
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        k, h, text = [], [], ""
        for _ in range(REPS):
            call()
            text = eng.lib.pe_last_error(eng.h).decode()
            k.append(float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)) * 1e3)
            h.append(float(re.search(r"plan_us=([0-9.]+)", text).group(1)))
            del os.environ["PE_CAP_EVENTS"]
            restore()
            os.environ["PE_CAP_EVENTS"] = "1"
        return median(k), median(h), text.split(" plan_us")[0]
    finally:
        os.environ.pop("PE_CAP_EVENTS", None)


def node_set(nodes, target):
    """The workaround: PE_NODE_SET of `nodes` with cap / used recomputed so that cap - used = target[:, nodes]."""
    t0 = time.perf_counter()
    cap = np.ascontiguousarray(inv.cap[:, nodes].T)
    used = np.ascontiguousarray(cap - target[:, nodes].T)
    lab = np.ascontiguousarray(inv.labels[nodes], np.uint32)
    isl = np.ascontiguousarray(island[nodes], np.int32)
    op = np.zeros(len(nodes), np.uint8)
    slots = np.ascontiguousarray(nodes, np.int64)
    prep = (time.perf_counter() - t0) * 1e6

    def call():
        rc = eng.lib.pe_update_nodes(eng.h, len(nodes), ptr(slots), ptr(op), ptr(cap), ptr(used), ptr(lab), ptr(isl))
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (cap, used, lab, isl, op, slots)
    return call, prep


for name, gangs, nodes in (("the whole placement", WHOLE, touched), ("one gang", ONE, one_touched)):
    with step(f"pe_release_gangs / pe_assume_gangs: {name}"):
        rel, ass = (lambda g=gangs: ledger("pe_release_gangs", g)), (lambda g=gangs: ledger("pe_assume_gangs", g))
        r_us = timed(rel, ass)
        rel()
        released = eng.read_residuals()                         # what the workaround has to write to give back
        a_us = timed(ass, rel)
        ass()
        assert np.array_equal(eng.read_residuals(), after), "release and assume must cancel"
        rk, rh, rt = inside(rel, ass)
        rel()
        ak, ah, at = inside(ass, rel)
        ass()
        print(f"{name}: {int(counted.value)} pods, {rt}", flush=True)
        print(f"  pe_release_gangs: call {r_us:.0f} us, host plan {rh:.0f} us, kernel {rk:.1f} us", flush=True)
        print(f"  pe_assume_gangs:  call {a_us:.0f} us, host plan {ah:.0f} us, kernel {ak:.1f} us", flush=True)
    with step(f"the workaround, pe_update_nodes with PE_NODE_SET: {name}"):
        give, prep_g = node_set(nodes, released)
        take, prep_t = node_set(nodes, after)
        g_us = timed(give, take)
        give()
        t_us = timed(take, give)
        print(f"  PE_NODE_SET of the same {len(nodes)} nodes: giving back {g_us:.0f} us, taking {t_us:.0f} us per call "
              f"(+ {max(prep_g, prep_t):.0f} us of numpy to recompute cap / used); the reset snapshot of the nodes is "
              f"overwritten", flush=True)
        print(f"  release {r_us / g_us:.2f} x, assume {a_us / t_us:.2f} x the workaround's call time", flush=True)
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)   # the snapshot back, and the placement assumed onto it
    ledger("pe_assume_gangs", WHOLE)
    assert np.array_equal(eng.read_residuals(), after)
eng.close()
