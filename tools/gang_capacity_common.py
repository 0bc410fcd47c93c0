"""What the three gang-capacity latency tools share (gang_capacity_latency.py, gang_capacity_domains_latency.py,
gang_capacity_tree_latency.py): the sizes read from the environment, the per-step watchdog, the raw C ABI call
of pe_gang_capacity and the kernels' hipEvent time."""
import ctypes
import faulthandler
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "training-operator_amd")]

P = ctypes.c_void_p
LIMIT = int(os.environ.get("GC_STEP_LIMIT_S", "120"))
NODES = int(os.environ.get("GC_NODES", "1000000"))
JOBS = int(os.environ.get("GC_JOBS", "100000"))


class step:
    """One GPU step under its own time limit: past it the watchdog thread dumps the stacks and exits."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        print(f"[{self.name}]", flush=True)
        faulthandler.dump_traceback_later(LIMIT, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def ptr(a):
    return None if a is None else a.ctypes.data_as(P)


def capacity_call(eng, req, need):
    req, need = np.ascontiguousarray(req, np.int64), np.ascontiguousarray(need, np.uint32)
    J = req.shape[0]
    slots, mx, nodes = np.zeros(J, np.int64), np.zeros(J, np.int32), np.zeros(J, np.int64)
    args = (eng.h, J, ptr(req), ptr(need), ptr(slots), ptr(mx), ptr(nodes))

    def call():
        rc = eng.lib.pe_gang_capacity(*args)
        assert rc == 0, eng.lib.pe_last_error(eng.h)
    call.keep = (req, need, slots, mx, nodes)
    return call


def kernel_ms(eng, call, reps, warm):
    """(median of the kernels' hipEvent time over `reps` calls, the call's distinct shapes): PE_CAP_EVENTS=1
    for these calls only, read back from pe_last_error."""
    os.environ["PE_CAP_EVENTS"] = "1"
    try:
        ms, shapes = [], None
        for i in range(warm + reps):
            call()
            m = re.match(r"S=(\d+) .*?kernels_ms=([0-9.]+)", eng.lib.pe_last_error(eng.h).decode())
            shapes = int(m.group(1))
            if i >= warm:
                ms.append(float(m.group(2)))
        return sorted(ms)[len(ms) // 2], shapes
    finally:
        del os.environ["PE_CAP_EVENTS"]
