"""pe_place_spread_domains on the device against the rule pod by pod in Python integers: every pod slot, status and
residual cell, exact.  The batches' zero-request group has 20 pods; test_literal_cases has the takes above 16 bits."""
import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import tree_capacity as TC
from oracle import semantics as S
from placement import PE_SPREAD_NODE, PE_SPREAD_NONE, Engine, _abi, synth

pytestmark = pytest.mark.gpu

GiB, ISLAND, BIG = DP.GiB, DP.ISLAND, 2**31 - 1
Q, QS, GPU1, ZERO, N = [16000, 64 * GiB, 0, 0], [500, GiB, 0, 0], [1000, GiB, 1, 0], [0, 0, 0, 0], PE_SPREAD_NODE
LIMIT = {"node": 928, "rack": 850}          # pe_kernels.h SP_LDS_NODES_NODE / SP_LDS_NODES_DOM


def spread_python(res, labels, island, batch, caps, spread_level, job_domain, level, level_size, parent):
    """(pods, status, residual [4][N]) by the rule of include/placement.h, one pod at a time: place_python's loop
    with a per-(group, spread domain) counter in the fit."""
    R = [[int(x) for x in row] for row in res]
    dom = DP.dom_level(island, level, level_size, parent)
    sd = list(range(len(dom))) if spread_level < 0 else DP.dom_level(island, spread_level, level_size, parent)
    poff = DP.pod_offsets(batch.group_count)
    pods, status = [-1] * poff[-1], [0] * len(batch.priority)
    for j in sorted(range(len(status)), key=lambda j: (-int(batch.priority[j]), j)):
        placed, cands = [], [n for n, d in enumerate(dom) if d == job_domain[j]]
        for g in range(int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])):
            q, need, c = [int(x) for x in batch.group_req[g]], int(batch.group_need[g]), int(batch.group_count[g])
            m = BIG if caps is None or caps[g] == PE_SPREAD_NONE else int(caps[g])
            unit = c if need & ISLAND else 1            # an island group: one step of `unit` pods
            qe, held = [x * unit for x in q], {}
            for p in range(0, c, unit):
                keys = [S.appendix_b_key([R[d][n] for d in range(4)], int(labels[n]), qe, need, n)
                        for n in cands if held.get(int(sd[n]), 0) + unit <= m]
                keys = [k for k in keys if k is not None] if max(qe) <= S.INT64_MAX else []
                if not keys:
                    break
                n = min(keys) & 0xFFFFFF
                held[int(sd[n])] = held.get(int(sd[n]), 0) + unit
                for d in range(4):
                    R[d][n] -= qe[d]
                pods[poff[g] + p:poff[g] + p + unit] = [n] * unit
                placed.append((g, n, unit))
            else:
                continue
            for g2, n, u in placed:                     # all or nothing
                for d in range(4):
                    R[d][n] += u * int(batch.group_req[g2][d])
            a, b = poff[int(batch.job_group_off[j])], poff[int(batch.job_group_off[j + 1])]
            pods[a:b], status[j] = [-1] * (b - a), 1
            break
    return np.array(pods, dtype=np.int32), np.array(status, dtype=np.int32), np.array(R, dtype=np.int64)


def make_case(size, kind, jobs, seed):
    """Domain 0 of `size` nodes and domain 1 of 5, dealt in a shuffled order, 3 nodes in no domain.  kind "node":
    one level, the cap per node.  kind "rack": the domains are blocks (level 1) over racks of unequal size -- a
    half, a quarter, an eighth and the rest of a block's nodes -- and the cap is per rack (spread_level 0)."""
    if kind == "node":
        return DP.one_level_case([size, 5], jobs, seed), PE_SPREAD_NODE
    rack_in = lambda k, s: min(3, int(np.log2(s / max(s - k, 1))))   # noqa: E731  (0: the first half, 1: the next quarter ...)
    racks = np.array([rack_in(k, size) for k in range(size)] + [4 + rack_in(k, 5) for k in range(5)] + [-1] * 3, np.int32)
    np.random.default_rng(seed).shuffle(racks)
    batch, job_domain = DP.make_batch(jobs)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(len(racks), seed), racks)
    return DP.Case(cap, used, labels, island, [8, 2], np.array([0] * 4 + [1] * 4, np.int32), 1, batch, job_domain), 0


def call(eng, case, caps, spread_level, dry_run=False):
    b = case.batch
    return eng.place_spread_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, caps,
                                    spread_level, case.job_domain, case.level, case.level_size, case.parent, dry_run)


def check(eng, case, caps, spread_level):
    before = eng.read_residuals()
    want = spread_python(before, case.labels, case.island, case.batch, caps, spread_level, case.job_domain, case.level,
                         case.level_size, case.parent)
    pods, st = call(eng, case, caps, spread_level)
    assert st.tolist() == want[1].tolist() and np.array_equal(pods, want[0]) and np.array_equal(eng.read_residuals(), want[2])
    return want


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# two jobs that take pods on several nodes and fail on their second group (3 pods: under a cap; 10: without one); a
# lower-priority job on what came back; island groups of 1 and 3 pods (cap >= count and cap < count under the caps 1
# and 2); a zero-request group whose cap is 2^31 - 1; a group of 7 whose cap fills a rack while other racks' nodes
# score worse; the small domain
NO_FIT = (1, [1, 0, 0, 0], DP.NO_LABEL)
JOBS = [(0, 9, [(3, Q, 0), NO_FIT]), (0, 9, [(10, Q, 0), NO_FIT]), (0, 8, [(3, Q, 0), (0, Q, 0)]), (0, 7, [(1, QS, ISLAND)]),
        (0, 7, [(3, QS, ISLAND)]), (0, 5, [(20, [0, 0, 0, 0], 0)]), (0, 4, [(7, QS, 0), (2, Q, 0)]), (1, 3, [(3, Q, 0)])]
CAPS = {"1": [1] * 12, "2": [2] * 12, "above": [100] * 12, "none": [PE_SPREAD_NONE] * 12,
        "mixed": [1, PE_SPREAD_NONE, 2, 100, 3, 2, 1, 2, BIG, 2, PE_SPREAD_NONE, 1]}
CAPS = {k: np.array(v[:8] + [BIG] + v[9:], dtype=np.int32) for k, v in CAPS.items()}   # group 8: the zero request
SIZES = [(0, 1), (0, 255), (0, 257), (1, -1), (1, 0), (1, 1)]   # (x the kind's LDS limit, +): limit + 1 is the global instance


@pytest.mark.parametrize("caps", list(CAPS))
@pytest.mark.parametrize("kind", ["node", "rack"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "limit%+d" % s[1] if s[0] else str(s[1]))
def test_against_the_rule(eng, size, kind, caps):
    size = size[0] * LIMIT[kind] + size[1]
    case, spread_level = make_case(size, kind, JOBS, seed=size)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    want = check(eng, case, CAPS[caps], spread_level)
    assert want[1][:2].tolist() == [1, 1] and (size == 1 or want[1][2] == 0)


@pytest.mark.parametrize("racks,level,spread_level,cap,count,q,pods", [   # 8 free GPUs a node: the header's examples
    ([0, 0], 0, N, PE_SPREAD_NONE, 4, GPU1, [0, 0, 0, 0]), ([0, 0], 0, N, 2, 4, GPU1, [0, 0, 1, 1]),
    ([0, 0], 0, N, 1, 4, GPU1, None), ([0, 0, 1, 1], 1, 0, 2, 4, GPU1, [0, 0, 2, 2]), ([0, 0, 1, 1], 1, 0, 1, 4, GPU1, None),
    ([0, 0], 0, N, 66000, 70000, ZERO, [0] * 66000 + [1] * 4000), ([0, 0], 0, N, BIG, 70000, ZERO, [0] * 70000),
    ([0, 0, 1], 1, 0, 66000, 70000, ZERO, [0] * 66000 + [2] * 4000)])   # takes and allowances above 16 bits
def test_literal_cases(eng, racks, level, spread_level, cap, count, q, pods):
    n = len(racks)
    free = np.array([[64000] * n, [256 << 30] * n, [8] * n, [0] * n], dtype=np.int64)
    batch, dom = DP.make_batch([(0, 0, [(count, q, 0)])])
    case = DP.Case(free, np.zeros_like(free), np.ones(n, dtype=np.uint32), np.array(racks, dtype=np.int32),
                   [1] if level == 0 else [2, 1], None if level == 0 else [0, 0], level, batch, dom)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    want = check(eng, case, [cap], spread_level)
    assert (want[0].tolist(), want[1].tolist()) == ((pods, [0]) if pods else ([-1] * count, [1]))


def test_identity_with_place_greedy_domains(eng):
    other = Engine(0)
    for level, spread_level, caps in ((0, N, None), (1, 0, True), (2, N, True), (2, 1, None)):
        case = DP.tree_case("racks32", 1025, level)
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
        other.load_nodes(case.cap, case.used, case.labels, case.island)
        b = case.batch
        want = other.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                          case.job_domain, level, case.level_size, case.parent)
        got = call(eng, case, caps and np.full(len(b.group_count), PE_SPREAD_NONE, dtype=np.int32), spread_level)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[1] == 0).any()
        assert np.array_equal(eng.read_residuals(), other.read_residuals())
    other.close()


@pytest.mark.parametrize("kind,size", [("node", 257), ("rack", 257), ("rack", 851)])
def test_dry_run_then_commit_then_release(eng, kind, size):
    case, spread_level = make_case(size, kind, JOBS, seed=size)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before, stats, held = eng.read_residuals(), eng.stats(), [x.copy() for x in eng.gang_capacity([Q, QS])]
    dry = call(eng, case, CAPS["2"], spread_level, dry_run=True)
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    assert all(np.array_equal(x, y) for x, y in zip(eng.gang_capacity([Q, QS]), held))
    got = call(eng, case, CAPS["2"], spread_level)
    assert np.array_equal(got[0], dry[0]) and np.array_equal(got[1], dry[1]) and (got[1] == 0).any() and (got[1] == 1).any()
    b = case.batch                                         # the ledger hand-over: the outputs as they are
    assert eng.release_gangs(b.job_group_off, b.group_count, b.group_req, got[0]) == int((got[0] >= 0).sum())
    assert np.array_equal(eng.read_residuals(), before)


def test_refusals():
    island, sizes, parent = TC.tree("racks32", 300)        # [10, 3, 1]
    inv = synth.make_inventory(300, 71)
    pods, st = np.full(6, -77, dtype=np.int32), np.full(2, -77, dtype=np.int32)   # sentinels
    good = dict(off=[0, 1, 3], pri=[0, 1], cnt=[2, 1, 3], req=[Q, QS, Q], cap=[1, -1, 2], sl=0, flags=0, dom=[1, 2], level=1,
                n_levels=3, sizes=sizes, parent=parent, n_jobs=2)

    def answers(e, code, text, **change):
        a = dict(good, **change)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int64 if k == "req" else np.int32)
               for k in ("off", "pri", "cnt", "req", "cap", "dom", "sizes", "parent")}
        ptr = lambda k: None if arr[k] is None else arr[k].ctypes.data   # noqa: E731
        rc = e.lib.pe_place_spread_domains(e.h, a["n_jobs"], ptr("off"), ptr("pri"), ptr("cnt"), ptr("req"), None, ptr("cap"),
                                           a["sl"], a["flags"], ptr("dom"), a["level"], a["n_levels"], ptr("sizes"),
                                           ptr("parent"), pods.ctypes.data, st.ctypes.data)
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg, change)
        assert ((pods == -77).all() and (st == -77).all()) == (code != _abi.PE_OK)   # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before, E = e.read_residuals(), _abi.PE_EINVAL
    for text, change in [("group_count: negative value at index 1", dict(cnt=[2, -1, 3])), ("n_jobs < 0", dict(n_jobs=-1)),
                         ("job_domain: value outside [0, level_size[level]) at index 1", dict(dom=[1, 3])),
                         ("level outside", dict(level=3)), ("parent is NULL", dict(parent=None)),
                         ("spread_level outside", dict(sl=-2)), ("spread_level outside", dict(sl=1)),
                         ("spread_level outside", dict(sl=0, level=0)),
                         ("group_max_per: value 0 or below -1 at index 2", dict(cap=[1, -1, 0])),
                         ("group_max_per: value 0 or below -1 at index 0", dict(cap=[-2, 0, 1])),
                         ("flags: unknown bits", dict(flags=2)), ("flags: unknown bits", dict(flags=0x80000001))]:
        answers(e, E, text, **change)
    assert np.array_equal(e.read_residuals(), before)
    for r in range(2):                                     # a 2-shard context
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(inv.cap, inv.used, inv.labels, island)
        answers(s, E, "shard")
        s.close()
    answers(e, _abi.PE_OK, "")                             # the same arguments unchanged are accepted
    e.close()
