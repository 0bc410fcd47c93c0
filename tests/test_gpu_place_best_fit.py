"""pe_place_best_fit_domains on the device against the rule stated job by job in Python integers: slots from
oracle.semantics' fit and floor division, the what-if and the placement from domain_placement.place_python.  Every
pod slot, status, job pair, pair-slots cell and residual is compared; the two identities are checked against the
engine's own calls; each refusal leaves residuals and outputs untouched."""
import numpy as np
import pytest

import domain_placement as DP
from oracle import semantics as S
from placement import PE_CAP_MAX, PE_PAIR_NO_FIT, PE_PAIR_REPEAT, Engine, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
ISLAND = DP.ISLAND
LDS = 1016                           # pe_kernels.h PL_LDS_NODES: the LDS instance's limit


def gpus(g):
    return [1000, GiB, g, 0]


def reference(res, labels, island, batch, pj, pd, n_dom):
    """(pods, status, pair, pair_slots, residual [4][N]): the rule of include/placement.h, job by job."""
    R = [[int(x) for x in row] for row in res]
    members = {}
    for n, d in enumerate(island):
        members.setdefault(int(d), []).append(n)
    jgo = [int(x) for x in batch.job_group_off]
    J = len(jgo) - 1
    poff = DP.pod_offsets(batch.group_count)
    pods, status, pair = [-1] * poff[-1], [1] * J, [-1] * J
    slots = [PE_PAIR_NO_FIT] * len(pj)

    def choose(j, state):
        groups = list(range(jgo[j], jgo[j + 1]))
        ref = max(groups, key=lambda g: (int(batch.group_count[g]), -g), default=None)
        if ref is not None and batch.group_count[ref] <= 0:
            ref = None
        one, _ = DP.make_batch([(0, 0, [(int(batch.group_count[g]), [int(x) for x in batch.group_req[g]],
                                         int(batch.group_need[g])) for g in groups])])
        best, seen = None, set()
        for p in [p for p in range(len(pj)) if pj[p] == j]:
            d = int(pd[p])
            if d in seen:
                slots[p] = PE_PAIR_REPEAT
                continue
            seen.add(d)
            s = 0
            if ref is not None:
                q, need = [int(x) for x in batch.group_req[ref]], int(batch.group_need[ref]) & ~ISLAND
                for n in members.get(d, []):
                    r4 = [state[k][n] for k in range(4)]
                    if S.appendix_b_key(r4, int(labels[n]), q, need, n) is not None:
                        s += min([PE_CAP_MAX] + [r // x for r, x in zip(r4, q) if x > 0])
            got = DP.place_python(state, labels, island, one, [d], 0, [n_dom], None)
            if got[1][0] == 0:
                slots[p] = s
                if best is None or s < best[0]:
                    best = (s, p, got[0], got[2])
        return best

    for j in sorted(range(J), key=lambda j: (-int(batch.priority[j]), j)):
        best = choose(j, R)
        if best is not None:
            _, pair[j], mine, R = best
            status[j] = 0
            pods[poff[jgo[j]]:poff[jgo[j + 1]]] = mine
    return pods, status, pair, slots, R


def hand_made(target, seed=5):
    """One level of 14 domains: 0 .. 12 small with hand-set free GPUs, 13 the TARGET of `target` nodes with 1 .. 8
    free GPUs each, and three nodes in no domain.  Returns (cap, labels, island, batch, pj, pd)."""
    small = [[8, 8], [8], [8], [8], [4, 4], [8, 8], [8], [8, 8], [8, 8, 8, 8], [3], [2], [4, 8], [8, 8]]
    T = len(small)
    rng = np.random.default_rng(seed)
    free = [g for d in small for g in d] + [int(x) for x in rng.integers(1, 9, target)] + [8, 8, 8]
    ids = [k for k, d in enumerate(small) for _ in d] + [T] * target + [-1] * 3
    order = rng.permutation(len(ids))
    free, island = np.array(free, dtype=np.int64)[order], np.array(ids, dtype=np.int32)[order]
    N = len(ids)
    cap = np.array([[64000] * N, [256 * GiB] * N, free, [0] * N], dtype=np.int64)
    labels = synth.island_labels(np.ones(N, dtype=np.uint32), island)
    jobs = [                                                      # (priority, groups, candidate domains)
        (10, [(4, gpus(1), 0)], [0, 1]),                          # 0: the header example: rack B (8) before rack A (16)
        (5, [(16, gpus(1), 0)], [0, 1]),                          # 1: ... which leaves rack A to this one
        (5, [(2, gpus(1), 0)], [3, 2, 3]),                        # 2: a tie on slots, decided by p; a repeated domain
        (5, [(6, gpus(1), 0), (1, gpus(3), 0)], [4, 5]),          # 3: 8 slots suffice, the second group does not fit
        (9, [(6, gpus(1), 0)], [6, 7]),                           # 4: takes domain 6, the tightest for job 5 too
        (1, [(4, gpus(1), 0)], [6, 7]),                           # 5: ... which now holds 2: domain 7
        (8, [(3, gpus(1), 0)], [T, 8]), (7, [(3, gpus(2), 0)], [8, T]), (6, [(5, gpus(1), 0)], [T]),
        (6, [(2, gpus(4), 0)], [T, 8]), (4, [(9, gpus(1), 0)], [T]),      # 6 .. 10: five jobs chained through T
        (3, [(2, gpus(1), 0)], [9]), (3, [(2, gpus(1), 0)], [10]),        # 11, 12: disjoint candidates
        (3, [(1, gpus(1), 0)], []),                               # 13: in no pair
        (2, [(100, gpus(1), 0)], [9, 10, 4]),                     # 14: fits nowhere
        (2, [(3, gpus(2), ISLAND), (1, gpus(1), 0)], [12, 11]),   # 15: an island reference group
    ]
    batch, _ = DP.make_batch([(0, p, g) for p, g, _ in jobs])
    # ungrouped: every job's k-th candidate before any job's next one, so each job's own order is kept
    pairs = [(j, c[k]) for k in range(3) for j, (_, _, c) in enumerate(jobs) if k < len(c)]
    pj, pd = np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32)
    return cap, labels, island, batch, pj, pd


N_DOM = 14


def call(e, batch, pj, pd, **kw):
    return e.place_best_fit_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                    batch.group_need, pj, pd, 0, [N_DOM], None, **kw)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    made = {target: hand_made(target) for target in (1, 2, LDS - 1, LDS, LDS + 1)}
    return {t: (c, reference(c[0], c[1], c[2], c[3], c[4], c[5], N_DOM)) for t, c in made.items()}


def test_the_hand_made_batch_reaches_its_cases(cases):
    (cap, labels, island, batch, pj, pd), (pods, status, pair, slots, R) = cases[2]
    dom = lambda j: -1 if pair[j] < 0 else int(pd[pair[j]])   # noqa: E731
    of = lambda j: [p for p in range(len(pj)) if pj[p] == j]  # noqa: E731
    assert (dom(0), dom(1)) == (1, 0) and status[:2] == [0, 0]                     # the header example
    assert slots[of(2)[0]] == slots[of(2)[1]] == 8 and pair[2] == of(2)[0]         # a tie, decided by p
    assert slots[of(2)[2]] == PE_PAIR_REPEAT                                       # a repeated domain
    assert slots[of(3)[0]] == PE_PAIR_NO_FIT and dom(3) == 5                       # slots 8 >= 7 pods, no fit
    assert dom(4) == 6 and slots[of(5)[0]] == PE_PAIR_NO_FIT and dom(5) == 7       # alone, job 5 had domain 6 (8 < 16)
    assert all(13 in pd[of(j)] for j in range(6, 11)) and {8, 13} <= {dom(j) for j in range(6, 11)}   # the chain
    assert (dom(11), dom(12)) == (9, 10)                                           # disjoint candidates
    assert status[13] == 1 and pair[13] == -1 and status[14] == 1 and pair[14] == -1
    assert [slots[p] for p in of(14)] == [PE_PAIR_NO_FIT] * 3
    assert dom(15) == 11 and slots[pair[15]] == 6 and slots[of(15)[0]] == 8        # the island reference group


@pytest.mark.parametrize("dry_run", [False, True])
@pytest.mark.parametrize("target", [1, 2, LDS - 1, LDS, LDS + 1])
def test_every_cell_against_the_rule(eng, cases, target, dry_run):
    (cap, labels, island, batch, pj, pd), want = cases[target]
    eng.load_nodes(cap, np.zeros_like(cap), labels, island)
    eng.reset_stats()
    got = call(eng, batch, pj, pd, dry_run=dry_run)
    for g, w in zip(got, want[:4]):
        assert g.tolist() == list(w)
    assert np.array_equal(eng.read_residuals(), cap if dry_run else np.array(want[4], dtype=np.int64))
    assert eng.stats()["jobs_placed"] == (0 if dry_run else want[1].count(0))
    eng.reset_residuals()                                          # twice, with a reset between: equal outputs
    again = call(eng, batch, pj, pd, dry_run=dry_run)
    assert all(np.array_equal(a, g) for a, g in zip(again, got))


def test_one_pair_per_job_is_place_greedy_domains(eng, cases):
    (cap, labels, island, batch, _, _), _ = cases[LDS + 1]
    J = len(batch.priority)
    job_domain = np.array([13, 8, 13, 4, 13, 6, 13, 8, 13, 13, 8, 9, 10, 2, 9, 11], dtype=np.int32)
    order = np.random.default_rng(1).permutation(J).astype(np.int32)
    eng.load_nodes(cap, np.zeros_like(cap), labels, island)
    pods, st, pair, slots = call(eng, batch, order, job_domain[order])
    after = eng.read_residuals()
    eng.reset_residuals()
    w_pods, w_st = eng.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count, batch.group_req,
                                            batch.group_need, job_domain, 0, [N_DOM], None)
    assert np.array_equal(pods, w_pods) and np.array_equal(st, w_st) and np.array_equal(eng.read_residuals(), after)
    assert (st == 0).any() and (st == 1).any()
    assert np.array_equal(pair, np.where(st == 0, np.argsort(order), -1)) and ((slots >= 0) == (st[order] == 0)).all()


@pytest.mark.parametrize("j", [3, 15, 14])
def test_one_job_is_the_argmin_of_capacity_over_the_pairs_that_fit(eng, cases, j):
    (cap, labels, island, batch, pj, pd), _ = cases[2]
    g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
    one = (np.array([0, g1 - g0], dtype=np.int32), [0], batch.group_count[g0:g1], batch.group_req[g0:g1], batch.group_need[g0:g1])
    mine = pd[pj == j]
    eng.load_nodes(cap, np.zeros_like(cap), labels, island)
    fits = eng.gang_fit_domains(one[0], *one[2:], np.zeros(len(mine), dtype=np.int32), mine, 0, [N_DOM]).fits
    ref = int(np.argmax(one[2]))
    table = eng.gang_capacity_domains(one[3][ref:ref + 1], one[4][ref:ref + 1] & np.uint32(~ISLAND & 0xFFFFFFFF), None,
                                      N_DOM).dom_slots[0]
    held = [(int(table[d]), p) for p, d in enumerate(mine) if fits[p]]
    _, st, pair, slots = eng.place_best_fit_domains(*one, np.zeros(len(mine), dtype=np.int32), mine, 0, [N_DOM], dry_run=True)
    assert pair.tolist() == [min(held)[1] if held else -1] and st.tolist() == [0 if held else 1]
    assert slots.tolist() == [int(table[d]) if fits[p] else PE_PAIR_NO_FIT for p, d in enumerate(mine)]


def test_refusals(cases):
    (cap, labels, island, batch, pj, pd), _ = cases[1]
    P, J = int(batch.group_count.sum()), len(batch.priority)
    outs = [np.full(P, -77, dtype=np.int32), np.full(J, -77, dtype=np.int32), np.full(J, -77, dtype=np.int32),
            np.full(len(pj), -77, dtype=np.int64)]
    sizes = np.array([N_DOM], dtype=np.int32)

    def answers(e, code, text, flags=0, level=0):
        rc = e.lib.pe_place_best_fit_domains(e.h, J, *(a.ctypes.data for a in (batch.job_group_off, batch.priority,
                                             batch.group_count, batch.group_req, batch.group_need)), len(pj), pj.ctypes.data,
                                             pd.ctypes.data, flags, level, 1, sizes.ctypes.data, None,
                                             *(o.ctypes.data for o in outs))
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert all((o == -77).all() for o in outs) == (code != _abi.PE_OK)     # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    e.load_nodes(cap, np.zeros_like(cap), labels, island)
    for text, change in [("flags: unknown bits", dict(flags=2)), ("flags: unknown bits", dict(flags=0x80000001)),
                         ("level outside", dict(level=1))]:
        answers(e, _abi.PE_EINVAL, text, **change)
    assert np.array_equal(e.read_residuals(), cap) and e.stats()["jobs_failed"] == 0
    s = Engine(0, rank=0, world_size=2, exchange=lambda b: b * 2)       # a 2-shard context
    s.load_nodes(cap, np.zeros_like(cap), labels, island)
    answers(s, _abi.PE_EINVAL, "shard")
    s.close()
    answers(e, _abi.PE_OK, "", flags=1)                                  # the same arguments are accepted
    e.close()
