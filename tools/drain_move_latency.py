#!/usr/bin/env python3
"""pe_drain_move_domains per-call latency on the cfg5 inventory (1M nodes), in one process, with
tools/drain_fit_latency.py's set-up and book: contiguous racks (n // 245) -> blocks -> zones -> root, the cfg3 batch
(10 000 jobs) as pe_place_greedy_domains placed it, and as candidates every node that holds a pod, each into its own
rack.  Median of N calls through the C ABI after 2 warm-ups, the state restored between calls (the ledger identity:
the moved slots released at their targets and assumed at their old nodes; checked once against the residuals read
back): the dry run and the committed call, each with its kernels alone (PE_CAP_EVENTS=1).  The yardstick, in the same
process: pe_drain_fit_domains on the same candidates.  The chain the call replaces -- pe_drain_fit_domains of one
node, pe_release_gangs, pe_assume_gangs -- is timed on a prefix of the candidates, per node.
    python tools/drain_move_latency.py     (GC_NODES / PD_JOBS / GC_RACK / PD_REPS / PD_CHAIN / GC_STEP_LIMIT_S to resize)"""
import os
import re
import time

import numpy as np

from gang_capacity_common import NODES, ptr, step   # (first: it sets the path)
from placement import Engine, synth  # noqa: E402

RACK = int(os.environ.get("GC_RACK", "245"))
JOBS = int(os.environ.get("PD_JOBS", "10000"))
REPS = int(os.environ.get("PD_REPS", "9"))
CHAIN = int(os.environ.get("PD_CHAIN", "50"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
batch = synth.make_jobs(JOBS, synth.SEED["cfg3"], "mixed")
island = (np.arange(NODES, dtype=np.int64) // RACK).astype(np.int32)
in_use = int(island.max()) + 1
racks = -(-in_use // 32) * 32
blocks = racks // 32
zones = -(-blocks // 32)
sizes = np.ascontiguousarray([racks, blocks, zones, 1], np.int32)
parent = np.ascontiguousarray(np.concatenate([np.arange(racks) // 32, np.arange(blocks) // 32, np.zeros(zones)]), np.int32)
jgo, pri = np.ascontiguousarray(batch.job_group_off, np.int32), np.ascontiguousarray(batch.priority, np.int32)
cnt, req = np.ascontiguousarray(batch.group_count, np.int32), np.ascontiguousarray(batch.group_req, np.int64)
need = np.ascontiguousarray(batch.group_need, np.uint32)
S = int(cnt.sum())

eng = Engine(0)
with step(f"load {NODES} nodes, racks of {RACK}"):
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
pods, status = np.full(max(S, 1), -1, np.int32), np.zeros(JOBS, np.int32)
spread = np.ascontiguousarray(np.arange(JOBS) % in_use, np.int32)
with step("pe_place_greedy_domains, spread racks: the resident book"):
    rc = eng.lib.pe_place_greedy_domains(eng.h, JOBS, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(spread), 0,
                                         len(sizes), ptr(sizes), ptr(parent), ptr(pods), ptr(status))
    assert rc == 0, eng.lib.pe_last_error(eng.h)
    cand_node = np.ascontiguousarray(np.unique(pods[pods >= 0]), np.int32)
    cand_domain = np.ascontiguousarray(island[cand_node], np.int32)
    C = len(cand_node)
    print(f"{JOBS} jobs, {S} pod slots, {int((pods >= 0).sum())} pods on {C} nodes in {len(np.unique(cand_domain))} racks, "
          f"at most {np.bincount(cand_domain).max()} candidates in one", flush=True)
    held = eng.read_residuals()
fits, moved = np.zeros(C, np.uint8), np.zeros(C, np.int64)
fail_slot, target = np.zeros(C, np.int64), np.zeros(max(S, 1), np.int32)
outs = (ptr(fits), ptr(moved), ptr(fail_slot), ptr(target))


def book(node, domain):
    return (eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(need), ptr(pods), len(node), ptr(node), ptr(domain), 0, len(sizes),
            ptr(sizes), ptr(parent))


def ok(rc):
    assert rc == 0, eng.lib.pe_last_error(eng.h)


def restore():
    old = np.ascontiguousarray(np.where(target >= 0, pods, -1), np.int32)
    ok(eng.lib.pe_release_gangs(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(target), None))
    ok(eng.lib.pe_assume_gangs(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(old), None))


def timed(call, after=None, events=False):
    """Median (us) of REPS calls after 2 warm-ups; events: the kernels alone, and the call's own report."""
    xs, text = [], ""
    if events:
        os.environ["PE_CAP_EVENTS"] = "1"
    try:
        for i in range(2 + REPS):
            eng.synchronize()
            t0 = time.perf_counter()
            call()
            us = (time.perf_counter() - t0) * 1e6
            if events:
                text = eng.lib.pe_last_error(eng.h).decode()
                us = float(re.search(r"kernels_ms=([0-9.]+)", text).group(1)) * 1e3
            if i >= 2:
                xs.append(us)
            if after:
                after()
    finally:
        os.environ.pop("PE_CAP_EVENTS", None)
    return median(xs), text.split(" kernels_ms")[0]


def fit_call():
    ok(eng.lib.pe_drain_fit_domains(*book(cand_node, cand_domain), *outs))


def move_call(flags):
    ok(eng.lib.pe_drain_move_domains(*book(cand_node, cand_domain), flags, *outs))


with step("pe_drain_fit_domains (the yardstick)"):
    f_us, _ = timed(fit_call)
    fk_us, ftext = timed(fit_call, events=True)
    f_fits = int(fits.sum())
    print(f"pe_drain_fit_domains: {C} candidates, {ftext}; call {f_us:.0f} us, kernels {fk_us:.0f} us; {f_fits} fit", flush=True)
with step("pe_drain_move_domains, dry run"):
    d_us, _ = timed(lambda: move_call(1))
    dk_us, dtext = timed(lambda: move_call(1), events=True)
    assert np.array_equal(eng.read_residuals(), held)
    print(f"pe_drain_move_domains dry: {dtext}; call {d_us:.0f} us, kernels {dk_us:.0f} us; {int(fits.sum())} fit, "
          f"{int(((fits == 0) & (moved > 0)).sum())} fail after moving a pod, {int((target[:S] >= 0).sum())} pods move", flush=True)
with step("pe_drain_move_domains, committed, the state restored between calls"):
    move_call(0)
    restore()
    assert np.array_equal(eng.read_residuals(), held)
    c_us, _ = timed(lambda: move_call(0), after=restore)
    ck_us, _ = timed(lambda: move_call(0), after=restore, events=True)
    print(f"pe_drain_move_domains committed: call {c_us:.0f} us, kernels {ck_us:.0f} us", flush=True)
with step(f"the three-call chain, node by node, on the first {CHAIN} candidates"):
    t0 = time.perf_counter()
    for c in range(min(CHAIN, C)):
        ok(eng.lib.pe_drain_fit_domains(*book(cand_node[c:c + 1], cand_domain[c:c + 1]), *outs))
        if fits[0]:
            restore_args = np.ascontiguousarray(np.where(target >= 0, pods, -1), np.int32)
            ok(eng.lib.pe_release_gangs(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(restore_args), None))
            ok(eng.lib.pe_assume_gangs(eng.h, JOBS, ptr(jgo), ptr(cnt), ptr(req), ptr(target), None))
    chain_us = (time.perf_counter() - t0) * 1e6 / max(1, min(CHAIN, C))
    print(f"chain: {chain_us:.0f} us per node ({chain_us * C / 1e3:.0f} ms for all {C} at that rate)", flush=True)
print(f"committed / yardstick: call {c_us / f_us:.3f}, kernels {ck_us / max(fk_us, 1e-9):.3f}; dry / yardstick: call "
      f"{d_us / f_us:.3f}, kernels {dk_us / max(fk_us, 1e-9):.3f}; per candidate {c_us / max(C, 1) * 1e3:.0f} ns", flush=True)
eng.close()
