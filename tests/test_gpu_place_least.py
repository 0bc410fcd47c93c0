"""pe_place_least_domains on the device against the rule one pod at a time in Python integers: every pod slot, status
and residual cell, exact.  The rule is place_python's loop with least_key built from oracle.semantics.appendix_b_key."""
import numpy as np
import pytest

import domain_placement as DP
from oracle import semantics as S
from placement import Engine, _abi, synth

pytestmark = pytest.mark.gpu

GiB, ISLAND = DP.GiB, DP.ISLAND
L = 843                                     # pe_kernels.h LS_LDS_NODES
SAT = S.SCORE_MAX + 1
ODD1, ODD3 = 0x5A5A5, 0xA5A5A5              # low bits of a memory and an ephemeral request: the >> 20 and >> 24 borrow
Q1, QB = [1000, GiB, 1, 0], [1000, GiB | ODD1, 0, GiB | ODD3]
NO_FIT = (1, [1, 0, 0, 0], DP.NO_LABEL)


def least_python(res, labels, island, batch, job_domain, level_size):
    """(pods, status, residual [4][N]) by the rule of include/placement.h, one pod at a time."""
    R = [[int(x) for x in row] for row in res]
    dom = DP.dom_level(island, 0, level_size, None)
    poff = DP.pod_offsets(batch.group_count)
    pods, status = [-1] * poff[-1], [0] * len(batch.priority)
    for j in sorted(range(len(status)), key=lambda j: (-int(batch.priority[j]), j)):
        placed, cands = [], [n for n, d in enumerate(dom) if d == job_domain[j]]
        for g in range(int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])):
            q, need, c = [int(x) for x in batch.group_req[g]], int(batch.group_need[g]), int(batch.group_count[g])
            unit = max(c, 1) if need & ISLAND else 1    # an island group: one step of `unit` pods
            qe = [x * unit for x in q]
            for p in range(0, c, unit):
                keys = [S.appendix_b_key([R[d][n] for d in range(4)], int(labels[n]), qe, need, n) for n in cands]
                keys = [((S.SCORE_MAX - (k >> 24)) << 24) | (k & 0xFFFFFF) for k in keys if k is not None]
                if not keys or max(qe) > S.INT64_MAX:
                    break
                n = min(keys) & 0xFFFFFF
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


def rack(size, seed):
    """(cap, labels, island): domain 0 of `size` nodes, domain 1 of 5, 3 nodes in no domain, ids shuffled.  Node k of
    domain 0 (ascending id) is, as far as the domain has it: k < 40 one of a LEVELLED set (label 2); 40..47 nodes
    with 8, 2, 2, 2, 1, 1, 1, 1 free GPUs (label 4: an empty node among full ones, nodes that no longer fit after a
    pod); 48..51 cpu alone, at and above the score's saturation line (label 8); 52..55 memory and ephemeral storage
    on both sides of QB's low bits (label 16); 56, 57, 58 three GPUs with 8M, 3M and 64 cpu (label 32: one Q1 pod
    lowers a score by 1 050 600, so 56 leads 57 and 57 leads 58 by more than the pods either holds); beyond, plain
    nodes whose cpu differs in five steps."""
    ids = np.array([0] * size + [1] * 5 + [-1] * 3, dtype=np.int32)
    np.random.default_rng(seed).shuffle(ids)
    cap = np.tile(np.array([[64000], [256 * GiB], [8], [100 * GiB]], dtype=np.int64), (1, len(ids)))
    lab = np.ones(len(ids), dtype=np.uint32)
    for k, n in enumerate(np.nonzero(ids == 0)[0]):
        if k < 40:
            lab[n] |= 2
        elif k < 48:
            lab[n], cap[2, n] = lab[n] | 4, [8, 2, 2, 2, 1, 1, 1, 1][k - 40]
        elif k < 52:
            lab[n], cap[:, n] = lab[n] | 8, [SAT + 1500 + 1100 * (k - 48), 0, 0, 0]
        elif k < 56:
            lab[n] |= 16
            cap[1, n], cap[3, n] = 64 * GiB + [0, ODD1 - 1, ODD1, ODD1 + 1][k - 52], 100 * GiB + [ODD3, ODD3 - 1, 0, ODD3 + 1][k - 52]
        elif k < 59:
            lab[n], cap[0, n], cap[2, n] = lab[n] | 32, [8000000, 3000000, 64000][k - 56], 3
        else:
            cap[0, n] -= 1000 * (k % 5)
    return cap, synth.island_labels(lab, ids), ids


def jobs_for(size):
    """Domain 0's jobs in priority order, each reaching what its comment names once the domain has the nodes."""
    m = min(size, 40)
    return [
        (0, 30, [(2 * m + 3, Q1, 2)]),                    # a levelled set: two whole layers, then a round cut by `left`
        (0, 29, [(14, Q1, 4)]),                           # a run ended by k2, rounds whose members stop fitting
        (0, 28, [(5, Q1, 32)]),                           # a run ended by take_of (3 on 56), one by `left` (2 on 57): k2 real
        (0, 27, [(12, [1000, 0, 0, 0], 8)]),              # saturated scores: ids decide; the last id's run crosses the line
        (0, 26, [(9, QB, 16)]),                           # the low-bit borrows of the memory and ephemeral terms
        (0, 25, [(70, [0, 0, 0, 0], 0)]),                 # a zero request: key == after, one run
        (0, 24, [(3, Q1, ISLAND | 2), (1, Q1, 2)]),       # an island group, then a pod
        (0, 23, [(2, Q1, 2), (3, [1 << 62, 0, 0, 0], ISLAND)]),   # an island product past int64: rolled back
        (0, 22, [(2 * m, Q1, 2), (2, Q1, 32), NO_FIT]),   # fails after two rounds and a run ...
        (0, 21, [(m, Q1, 2), (0, Q1, 0)]),                # ... and this one fits on what came back
        (0, 21, []), (1, 5, [(7, Q1, 0)]), (1, 6, [(4, Q1, ISLAND), (30, Q1, 0)]),   # the small domain: 40 GPUs
    ]


def call(eng, case, dry_run=False):
    b = case.batch
    return eng.place_least_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, case.job_domain,
                                   case.level, case.level_size, case.parent, dry_run)


def check(eng, case):
    before = eng.read_residuals()
    want = least_python(before, case.labels, case.island, case.batch, case.job_domain, case.level_size)
    pods, st = call(eng, case)
    assert st.tolist() == want[1].tolist() and np.array_equal(pods, want[0]) and np.array_equal(eng.read_residuals(), want[2])
    return want


def make_case(size, jobs=None):
    cap, labels, island = rack(size, seed=size)
    batch, job_domain = DP.make_batch(jobs_for(size) if jobs is None else jobs)
    return DP.Case(cap, np.zeros_like(cap), labels, island, [2], None, 0, batch, job_domain)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("size", [1, 2, 255, 256, 257, L - 1, L, L + 1])   # L + 1: the in-place instance
def test_against_the_rule(eng, size):
    case = make_case(size)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    want = check(eng, case)
    if size >= 255:                          # all placed but the two meant to fail and the small domain's second
        assert want[1].tolist() == [0] * 7 + [1, 1, 0, 0, 1, 0]
        layer = sorted(want[0][:40].tolist())
        assert sorted(want[0][40:80].tolist()) == layer and len(set(layer)) == 40   # two whole layers of the levelled set
        n56, n57 = np.nonzero(case.island == 0)[0][56:58].tolist()
        assert want[0][97:102].tolist() == [n56] * 3 + [n57] * 2                    # job 2: the two runs, not rounds
    mix, dom = DP.job_mix(eng.read_residuals(), case.labels, case.island, 0, [2], None, seed=size)   # on what is left
    check(eng, DP.Case(case.cap, case.used, case.labels, case.island, [2], None, 0, mix, dom))


def test_header_example(eng):
    free = np.array([[64000] * 2, [256 << 30] * 2, [8] * 2, [0] * 2], dtype=np.int64)
    batch, dom = DP.make_batch([(0, 0, [(4, Q1, 0)])])
    case = DP.Case(free, np.zeros_like(free), np.ones(2, dtype=np.uint32), np.zeros(2, dtype=np.int32), [1], None, 0, batch, dom)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    assert check(eng, case)[0].tolist() == [0, 1, 0, 1] and eng.read_residuals()[2].tolist() == [6, 6]


def test_round_above_the_rank_limit(eng):
    """7987 of the 8000 nodes lie below theta, more than a round ranks (pe_kernels.h LS_RANK_MAX = 4096): the
    first group's decisions are made as runs of one pod; the second group's 40 members are a round again."""
    case = make_case(8000, [(0, 1, [(10, Q1, 0), (43, Q1, 2)])])
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    assert check(eng, case)[1].tolist() == [0]


@pytest.mark.parametrize("size", [257, L + 1])
def test_dry_run_then_commit_then_release(eng, size):
    case = make_case(size)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before, stats = eng.read_residuals(), eng.stats()
    dry = call(eng, case, dry_run=True)
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    got = call(eng, case)
    assert np.array_equal(got[0], dry[0]) and np.array_equal(got[1], dry[1]) and (got[1] == 0).any() and (got[1] == 1).any()
    assert eng.stats() != stats and not np.array_equal(eng.read_residuals(), before)
    b = case.batch                                         # the ledger hand-over: the outputs as they are
    assert eng.release_gangs(b.job_group_off, b.group_count, b.group_req, got[0]) == int((got[0] >= 0).sum())
    assert np.array_equal(eng.read_residuals(), before)


def test_refusals():
    cap, labels, island = rack(300, seed=3)
    pods, st = np.full(6, -77, dtype=np.int32), np.full(2, -77, dtype=np.int32)   # sentinels
    good = dict(off=[0, 1, 3], pri=[0, 1], cnt=[2, 1, 3], req=[Q1, QB, Q1], flags=0, dom=[1, 0], level=0, n_levels=1,
                sizes=[2], n_jobs=2)

    def answers(e, code, text, **change):
        a = dict(good, **change)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int64 if k == "req" else np.int32)
               for k in ("off", "pri", "cnt", "req", "dom", "sizes")}
        ptr = lambda k: None if arr[k] is None else arr[k].ctypes.data   # noqa: E731
        rc = e.lib.pe_place_least_domains(e.h, a["n_jobs"], ptr("off"), ptr("pri"), ptr("cnt"), ptr("req"), None, a["flags"],
                                          ptr("dom"), a["level"], a["n_levels"], ptr("sizes"), None, pods.ctypes.data,
                                          st.ctypes.data)
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg, change)
        assert ((pods == -77).all() and (st == -77).all()) == (code != _abi.PE_OK)   # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    e.load_nodes(cap, np.zeros_like(cap), labels, island)
    before, E = e.read_residuals(), _abi.PE_EINVAL
    for text, change in [("group_count: negative value at index 1", dict(cnt=[2, -1, 3])), ("n_jobs < 0", dict(n_jobs=-1)),
                         ("job_domain: value outside [0, level_size[level]) at index 1", dict(dom=[1, 2])),
                         ("job_domain is NULL", dict(dom=None)), ("level outside", dict(level=1)),
                         ("parent is NULL", dict(n_levels=2, sizes=[2, 1])),
                         ("flags: unknown bits", dict(flags=2)), ("flags: unknown bits", dict(flags=0x80000001))]:
        answers(e, E, text, **change)
    assert np.array_equal(e.read_residuals(), before)
    for r in range(2):                                     # a 2-shard context
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(cap, np.zeros_like(cap), labels, island)
        answers(s, E, "shard")
        s.close()
    answers(e, _abi.PE_OK, "")                             # the same arguments unchanged are accepted
    e.close()
