#!/usr/bin/env python3
"""pe_gang_capacity per-call latency on the cfg5 inventory (1M nodes), in one process: median of N calls
through the C ABI after a warm-up.  Reports the call at J = 1, the call for the cfg5 batch (100 000
jobs, S distinct shapes), the one-shot pe_fit_mask on the same batch as the yardstick, and the
capacity kernels alone (PE_CAP_EVENTS=1: hipEvents on the context stream around the launches, read back
from pe_last_error).  Every step runs under a watchdog of its own that ends the process if it overruns.
    python tools/gang_capacity_latency.py            (GC_NODES / GC_JOBS / GC_STEP_LIMIT_S to resize)"""
import ctypes

import numpy as np

from gang_capacity_common import JOBS, NODES, P, capacity_call, kernel_ms, ptr, step   # (first: it sets the path)
import bench  # noqa: E402
from placement import Engine, synth  # noqa: E402


def fit_call(eng, req, need):
    req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
    counts = np.zeros(req.shape[0], np.int64)
    dptr, wpr = P(), ctypes.c_int64()
    args = (eng.h, req.shape[0], ptr(req), ptr(need), ptr(counts), ctypes.byref(dptr), ctypes.byref(wpr))

    def call():
        assert eng.lib.pe_fit_mask(*args) == 0
    call.keep = (req, need, counts)
    return call


seed = synth.SEED["cfg5"]
with step(f"load {NODES} nodes"):
    eng = Engine(0)
    inv = synth.make_inventory(NODES, seed, 0.2)
    eng.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
req, need = synth.make_fit_jobs(JOBS, seed)

with step("J = 1"):
    one = capacity_call(eng, req[:1], need[:1])
    med, p90 = bench.time_calls(one, 500, 30)
    k1, _ = kernel_ms(eng, one, 100, 10)
    print(f"pe_gang_capacity J 1: call {med:.1f} us (p90 {p90:.1f}), kernels {k1 * 1e3:.1f} us", flush=True)

with step(f"J = {JOBS}"):
    full = capacity_call(eng, req, need)
    med, p90 = bench.time_calls(full, 20, 3)
    kf, shapes = kernel_ms(eng, full, 10, 2)
    print(f"pe_gang_capacity J {JOBS}: S {shapes} shapes, call {med:.1f} us (p90 {p90:.1f}), kernels {kf * 1e3:.1f} us",
          flush=True)

with step("pe_fit_mask, one-shot, same batch"):
    fit = fit_call(eng, req, need)
    med, p90 = bench.time_calls(fit, 20, 3)
    print(f"pe_fit_mask J {JOBS}: call {med:.1f} us (p90 {p90:.1f})", flush=True)

with step("pe_gang_capacity again (run-to-run noise)"):
    med, p90 = bench.time_calls(full, 20, 3)
    print(f"pe_gang_capacity J {JOBS}: call {med:.1f} us (p90 {p90:.1f})", flush=True)
eng.close()
