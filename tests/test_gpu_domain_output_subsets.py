"""The judging domain calls (gang-fit, gang-preempt, drain-fit, scale-up) copy back one span of their answer block:
from the first to the last answer the caller asked for.  Every non-empty proper subset of each call's optional
outputs must return, for the parts it asks for, what the call with every output returns -- on one context, on a
48-node inventory in two racks of 24.  The pinned answer buffer outlives a call, so a span cut too short would hand
back what the call before left there: every subset call follows a call of the same shape whose every part differs
(the groups ask for a label that no node carries), and a part that did not cross shows as that call's."""
import itertools

import numpy as np
import pytest

from placement import Engine

pytestmark = pytest.mark.gpu

GiB = 1 << 30
N, RACK = 48, 24
SIZES = np.array([2], dtype=np.int32)            # one level: the two racks
VIC_NODES = np.array([0, 1, 24, 25], dtype=np.int32)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def load(e):
    """Nodes of 8 GPUs with 0..7 in use, cpu and memory ample; two placed gangs of two 8-GPU pods fill nodes 0, 1 and
    24, 25.  Each rack is left with two more empty nodes."""
    n = np.arange(N)
    cap = np.zeros((4, N), dtype=np.int64)
    cap[0], cap[1], cap[2] = 64000, 256 * GiB, 8
    used = np.zeros((4, N), dtype=np.int64)
    used[2] = np.where(n < RACK, n % 8, (n * 3) % 8)
    used[2, VIC_NODES] = 8
    e.load_nodes(cap, used, np.zeros(N, dtype=np.uint32), (n // RACK).astype(np.int32))


def gpus(g):
    return [1000, GiB, g, 0]


# 3 jobs of 1 to 2 groups: 4 x 2 GPUs; 3 x 4 GPUs and 2 x 1 GPU; 4 whole nodes (two more than a rack has empty)
JGO = np.array([0, 1, 3, 4], dtype=np.int32)
CNT = np.array([4, 3, 2, 4], dtype=np.int32)
REQ = np.array([gpus(2), gpus(4), gpus(1), gpus(8)], dtype=np.int64)
NEED = np.zeros(4, dtype=np.uint32)
NO_NODE = np.ones(4, dtype=np.uint32)            # a label bit no node carries: nothing fits anywhere
PAIR_JOB = np.array([0, 0, 1, 1, 2], dtype=np.int32)
PAIR_DOM = np.array([0, 1, 0, 1, 1], dtype=np.int32)
J, P = 3, 5
# the two placed gangs: the victims of the preempt call, the book of the drain call
VGO = np.array([0, 1, 2], dtype=np.int32)
VCNT = np.array([2, 2], dtype=np.int32)
VREQ = np.array([gpus(8), gpus(8)], dtype=np.int64)
PAIR_VIC_OFF = np.arange(0, 2 * P + 1, 2, dtype=np.int32)
PAIR_VIC = np.array([0, 1] * P, dtype=np.int32)


def proper_subsets(n):
    """Every non-empty proper subset of n outputs, as tuples of booleans."""
    return [w for w in itertools.product([False, True], repeat=n) if any(w) and not all(w)]


def differ(poison, full, what):
    """The call before a subset call: all of its parts are there, and none equals the part under test."""
    for g, f, name in zip(poison, full, what):
        assert g.shape == f.shape and g.dtype == f.dtype and not np.array_equal(g, f), name


def same_parts(got, full, want, what):
    for g, f, w, name in zip(got, full, want, what):
        if w:
            assert g is not None and g.dtype == f.dtype and np.array_equal(g, f), (name, want)
        else:
            assert g is None, (name, want)


def ptr(a):
    return None if a is None else a.ctypes.data


def test_gang_fit_output_subsets(eng):
    load(eng)
    full = eng.gang_fit_domains(JGO, CNT, REQ, NEED, PAIR_JOB, PAIR_DOM, 0, SIZES)
    assert full.fits.tolist() == [1, 1, 1, 1, 0] and full.first.tolist() == [0, 2, -1]
    names = ("fits", "fail_group", "pods", "first")
    for want in proper_subsets(4):      # the binding has one switch for the three tables: the entry point itself
        differ(eng.gang_fit_domains(JGO, CNT, REQ, NO_NODE, PAIR_JOB, PAIR_DOM, 0, SIZES), full, names)
        outs = [np.zeros(P, np.uint8), np.full(P, -1, np.int32), np.zeros(P, np.int64), np.full(J, -1, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        rc = eng.lib.pe_gang_fit_domains(eng.h, J, ptr(JGO), ptr(CNT), ptr(REQ), ptr(NEED), P, ptr(PAIR_JOB), ptr(PAIR_DOM),
                                         0, 1, ptr(SIZES), None, *[ptr(o) for o in outs])
        assert rc == 0, eng.lib.pe_last_error(eng.h)
        same_parts(outs, full, want, names)
    for kw, want in (({"tables": False}, (False, False, False, True)), ({"first": False}, (True, True, True, False))):
        differ(eng.gang_fit_domains(JGO, CNT, REQ, NO_NODE, PAIR_JOB, PAIR_DOM, 0, SIZES), full, names)
        same_parts(eng.gang_fit_domains(JGO, CNT, REQ, NEED, PAIR_JOB, PAIR_DOM, 0, SIZES, **kw), full, want, names)


def test_gang_preempt_output_subsets(eng):
    load(eng)
    args = (JGO, CNT, REQ, NEED, VGO, VCNT, VREQ, VIC_NODES, PAIR_JOB, PAIR_DOM, PAIR_VIC_OFF, PAIR_VIC, 0, SIZES)
    other = args[:3] + (NO_NODE,) + args[4:]
    full = eng.gang_preempt_domains(*args)
    assert full.count.tolist() == [0, 0, 0, 0, 1] and full.best.tolist() == [0, 2, 4]   # job 2: victim 1 has to go
    names = ("prefix", "victims", "count", "best")
    for want in proper_subsets(4):      # the binding has one switch for the three tables: the entry point itself
        differ(eng.gang_preempt_domains(*other), full, names)
        outs = [np.full(P, -1, np.int32), np.zeros(P, np.uint64), np.full(P, -1, np.int32), np.full(J, -1, np.int32)]
        outs = [o if w else None for o, w in zip(outs, want)]
        rc = eng.lib.pe_gang_preempt_domains(eng.h, J, ptr(JGO), ptr(CNT), ptr(REQ), ptr(NEED), 2, ptr(VGO), ptr(VCNT),
                                             ptr(VREQ), ptr(VIC_NODES), P, ptr(PAIR_JOB), ptr(PAIR_DOM), ptr(PAIR_VIC_OFF),
                                             ptr(PAIR_VIC), 0, 1, ptr(SIZES), None, *[ptr(o) for o in outs])
        assert rc == 0, eng.lib.pe_last_error(eng.h)
        same_parts(outs, full, want, names)
    for kw, want in (({"tables": False}, (False, False, False, True)), ({"best": False}, (True, True, True, False))):
        differ(eng.gang_preempt_domains(*other), full, names)
        same_parts(eng.gang_preempt_domains(*args, **kw), full, want, names)


def test_drain_fit_output_subsets(eng):
    load(eng)
    cand_dom = np.array([0, 1, 1, 0], dtype=np.int32)     # 4 candidates: each gang node, to its own or the other rack
    args = (VGO, VCNT, VREQ, np.zeros(2, np.uint32), VIC_NODES, VIC_NODES, cand_dom, 0, SIZES)
    other = args[:3] + (np.ones(2, np.uint32),) + args[4:]
    full = eng.drain_fit_domains(*args)
    assert full.fits.tolist() == [1, 1, 1, 1] and full.moved.tolist() == [1, 1, 1, 1] and (full.target >= 0).all()
    names = ("fits", "moved", "fail_slot", "target")
    for want in proper_subsets(4):
        differ(eng.drain_fit_domains(*other), full, names)
        got = eng.drain_fit_domains(*args, fits=want[0], moved=want[1], fail_slot=want[2], target=want[3])
        same_parts(got, full, want, names)


def test_scale_up_output_subsets(eng):
    load(eng)
    slots = np.array([23, 47], dtype=np.int32)            # the last node of each rack goes: the new nodes' slots
    eng.update_nodes(slots, [1, 1])
    tmpl = np.array([[64000, 256 * GiB, 8, 0]], dtype=np.int64)
    args = (JGO, CNT, REQ, NEED, tmpl, None, slots, PAIR_JOB, PAIR_DOM, np.zeros(P, np.int32), None, 0, SIZES)
    other = args[:3] + (NO_NODE,) + args[4:]
    full = eng.scale_up_domains(*args)
    assert full.nodes.tolist() == [0, 0, 0, 0, 2] and full.best.tolist() == [0, 2, 4]
    names = ("nodes", "fail_group", "pods", "new_pods", "best")
    for want in proper_subsets(5):
        differ(eng.scale_up_domains(*other), full, names)
        got = eng.scale_up_domains(*args, nodes=want[0], fail_group=want[1], pods=want[2], new_pods=want[3], best=want[4])
        same_parts(got, full, want, names)
