"""pe_place_first_fit_domains on the CPU: the three statements of the rule in tests/first_fit.py agree on every
named hierarchy and level, the round scheme stays within its bound and does not depend on the order in which the
domains take their turn, the shared cases show what they are meant to show, the two identities of the header, the
traps by hand, and the bindings."""
import re

import numpy as np
import pytest

import domain_placement as DP
import first_fit as FF
import gang_fit as GF
import tree_capacity as TC
from placement import Engine, _abi

SIZES = (257, 1025)
TREE_LEVELS = [(name, n, level) for name in TC.TREES for n in SIZES for level in DP.tree_levels(name, n)]
# levels of ONE domain: every pair names that domain, and what the first pair of a job could not do no later pair can
ONE_DOMAIN = {(name, n, level) for name, n, level in TREE_LEVELS if TC.tree(name, n)[1][level] == 1}


def args_of(c, pj, pd):
    return (c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)


@pytest.fixture(scope="module")
def cases():
    """The case, its pairs and the sequential answer per (tree, n, level), computed once."""
    out = {}
    for name, n, level in TREE_LEVELS:
        c, pj, pd = FF.pairs_case(name, n, level)
        out[name, n, level] = (c, pj, pd, FF.place_first_fit(*args_of(c, pj, pd)))
    return out


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_three_statements_agree(cases, name, n, level):
    c, pj, pd, want = cases[name, n, level]
    model = FF.rounds_model(*args_of(c, pj, pd))
    assert same(want, model)
    assert 1 <= model[4] <= len(pj) + 1
    back = FF.rounds_model(*args_of(c, pj, pd), reverse=True)
    assert same(want, back) and back[4] == model[4]          # whichever domain goes first
    if n == 257:
        assert same(want, FF.place_first_fit_python(*args_of(c, pj, pd)))


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_cases_are_not_vacuous(cases, name, n, level):
    c, pj, pd, (pods, status, pair, res) = cases[name, n, level]
    J = len(status)
    cand = FF.candidates(pj, J)
    assert not (np.diff(pj) >= 0).all()                                          # not grouped by job
    assert not cand[J - 5] and status[J - 5] == 1 and pair[J - 5] == -1            # a job in no pair
    assert (status == 0).any() and ((pair >= 0) == (status == 0)).all()
    assert any(status[j] == 1 and cand[j] for j in range(J))                     # candidates, and none fits
    later = any(pair[j] >= 0 and pair[j] != cand[j][0] for j in range(J))        # placed by a pair that is not its first
    assert later == ((name, n, level) not in ONE_DOMAIN), (name, n, level)
    # a job whose pair differs from its first fit on the untouched residuals: an earlier job took the room
    fits, _, _ = GF.answers(*args_of(c, pj, pd)[:3], c.batch, pj, pd, c.level, c.level_size, c.parent)
    alone = GF.first_of(pj, fits, J)
    assert any(cand[j] and pair[j] != alone[j] for j in range(J))


def test_identity_one_pair_per_job(cases):
    """With exactly one pair per job every output equals pe_place_greedy_domains with that pair's domain."""
    for key in (("permuted", 257, 0), ("four", 1025, 1)):
        c = cases[key][0]
        J = len(c.batch.job_group_off) - 1
        order = np.random.default_rng(3).permutation(J).astype(np.int32)     # pair p belongs to job order[p]
        pd = c.job_domain[order]
        got = FF.place_first_fit(*args_of(c, order, pd))
        pods, status, res = DP.place(c.residual(), c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent)
        assert np.array_equal(got[0], pods) and np.array_equal(got[1], status) and np.array_equal(got[3], res)
        inv = np.empty(J, dtype=np.int32)
        inv[order] = np.arange(J, dtype=np.int32)
        assert np.array_equal(got[2], np.where(status == 0, inv, -1))
        assert (status == 0).any() and (status == 1).any()


def test_identity_one_job(cases):
    """With one job in the call out_job_pair[0] is pe_gang_fit_domains' out_first[0] on the same residuals."""
    c, pj, pd, _ = cases["permuted", 257, 1]
    seen = set()
    for j in range(len(c.batch.job_group_off) - 1):
        one = FF.single_job(c.batch, j)
        mine = pd[pj == j]
        zeros = np.zeros(len(mine), dtype=np.int32)
        got = FF.place_first_fit(c.residual(), c.labels, c.island, one, zeros, mine, c.level, c.level_size, c.parent)
        fits, _, _ = GF.answers(c.residual(), c.labels, c.island, one, zeros, mine, c.level, c.level_size, c.parent)
        first = GF.first_of(zeros, fits, 1)
        assert got[2].tolist() == first.tolist()
        seen.add(-1 if first[0] < 0 else min(int(first[0]), 1))
    assert seen == {-1, 0, 1}                                # no fit, the first pair, a later pair


def all_statements(case, pj, pd):
    want = FF.place_first_fit(*args_of(case, pj, pd))
    assert same(want, FF.place_first_fit_python(*args_of(case, pj, pd)))
    model = FF.rounds_model(*args_of(case, pj, pd))
    back = FF.rounds_model(*args_of(case, pj, pd), reverse=True)
    assert same(want, model) and same(want, back) and model[4] == back[4] <= len(pj) + 1
    return want, model[4]


def test_trap_priority():
    (pods, status, pair, _), rounds = all_statements(*FF.trap_priority())
    w = FF.TRAP_PRIORITY_WANT
    assert pods.tolist() == w["pods"] and status.tolist() == w["status"] and pair.tolist() == w["pair"]
    assert rounds == 2                                       # A fails in domain 1, then takes domain 2; B waits behind it


def test_trap_chain():
    (pods, status, pair, _), rounds = all_statements(*FF.trap_chain())
    w = FF.TRAP_CHAIN_WANT
    assert pods.tolist() == w["pods"] and status.tolist() == w["status"] and pair.tolist() == w["pair"]
    assert rounds == w["rounds"]


def test_trap_repeat():
    case, pj, pd = FF.trap_repeat()
    (pods, status, pair, res), rounds = all_statements(case, pj, pd)
    w = FF.TRAP_REPEAT_WANT
    assert status.tolist() == w["status"] and pair.tolist() == w["pair"] and rounds == 3
    assert set(pods[:5].tolist()) <= {2, 3, 4} and sorted(pods[5:].tolist()) == [0, 1]   # B has rack 0 to itself
    assert res[2][:2].tolist() == [0, 0] and int(res[2][2:].sum()) == 24 - 16


def test_trap_all_one_domain():
    case, pj, pd = FF.trap_all_one_domain()
    want = FF.place_first_fit(*args_of(case, pj, pd))
    model = FF.rounds_model(*args_of(case, pj, pd))
    assert same(want, model) and model[4] == 1               # one queue: fully sequential, one round
    assert (want[1] == 0).any() and (want[1] == 1).any()
    # a job alone is place_greedy_domains' job: the whole batch is that call with every job in domain 0
    pods, status, res = DP.place(case.residual(), case.labels, case.island, case.batch, case.job_domain, 0, case.level_size, None)
    assert np.array_equal(want[0], pods) and np.array_equal(want[1], status) and np.array_equal(want[3], res)


@pytest.mark.parametrize("big", [65, 1017])
def test_overflow_cases_overflow_both_ways(big):
    case, pj, pd = FF.overflow_case(big)
    want = FF.place_first_fit(*args_of(case, pj, pd))
    assert FF.overflow_conditions(pj, pd, want[2]) == (True, True)
    assert same(want, FF.rounds_model(*args_of(case, pj, pd)))


def test_bindings():
    sig = _abi.SIGNATURES["pe_place_first_fit_domains"]
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pe_place_first_fit_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "pe_place_first_fit_domains is not declared in placement.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig[1]) == 17
    P, i32, i64 = _abi.P, _abi.i32, _abi.i64
    for p, t in zip(params, sig[1]):
        want = P if "*" in p else i64 if p.startswith("int64_t") else i32
        assert t is want, (p, t)
    assert callable(getattr(Engine, "place_first_fit_domains"))
