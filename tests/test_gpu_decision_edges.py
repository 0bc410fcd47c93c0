"""The five domain calls on the device over the edge cases of tests/decision_edges.py: every output cell of every
call against that call's checker (check_engine in domain_placement.py, gang_fit.py, first_fit.py, min_member.py and
gang_preempt.py), residuals read back after every call.  Each call meets the small domain (working state in LDS),
the domain of 1017 nodes (global memory) and the empty one.  What the cases show is asserted on the CPU
(test_decision_edges_cpu.py); here only what a call adds."""
import numpy as np
import pytest

import decision_edges as DE
import domain_placement as DP
import first_fit as FF
import gang_fit as GF
import gang_preempt as GP
import min_member as MM
from placement import Engine

pytestmark = pytest.mark.gpu

# the zero-request group of the pe_place_greedy_domains batch, one take on the device: 100 000 pods in the small
# domain and 500 in the large one (the checker places them one by one over every node of the domain)
ZERO = (100_000, 500)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def greedy(eng):
    """The edge batch through pe_place_greedy_domains on the fresh inventory: (EdgeCase, the checker's answer)."""
    ec = DE.edge_case(ZERO)
    return ec, DP.check_engine(eng, ec.case)


def test_greedy_domains_and_again_without_reset(eng, greedy):
    ec, (pods, st, res) = greedy
    for d in (DE.SMALL, DE.LARGE):
        mine = ec.case.job_domain == d
        assert (st[mine] == 0).sum() > 30 and (st[mine] == 1).sum() >= 4
        (j,) = ec.jobs_named("zero", d)
        g = int(ec.case.batch.job_group_off[j])
        p0 = DP.pod_offsets(ec.case.batch.group_count)[g]
        assert len(set(pods[p0:p0 + ZERO[d]].tolist())) == 1 and pods[p0] >= 0
    assert [int(st[j]) for n in ("empty_pod", "empty_none", "empty_island") for j in ec.jobs_named(n)] == [1, 0, 1]
    assert np.array_equal(eng.read_residuals(), res)
    again = DP.check_engine(eng, ec.case, load=False)        # the checker starts from read_residuals()
    assert again[1].tolist() != st.tolist() and not np.array_equal(again[2], res)


def test_gang_fit(eng):
    ec = DE.edge_case()
    pj, pd = DE.fit_pairs(ec)
    fits, fail, pods, first = GF.check_engine(eng, ec.case, pj, pd)
    for d in (DE.SMALL, DE.LARGE):                           # both instances say yes and no
        assert set(fits[pd == d].tolist()) == {0, 1}
    assert set(pd.tolist()) == {DE.SMALL, DE.LARGE, DE.EMPTY} and (fail >= 1).any()


def test_first_fit(eng):
    ec, pj, pd = DE.first_fit_case()
    pods, st, pair, _ = FF.check_engine(eng, ec.case, pj, pd)
    assert DE.first_fit_crossed(ec, pj, pd, st, pair)
    (j,) = ec.jobs_named("hopeless")
    assert st[j] == 1 and pair[j] == -1


def test_min_member_all_is_greedy_domains(eng, greedy):
    ec, (pods, st, res) = greedy
    _, cases = DE.min_member_cases(ZERO)
    want = MM.check_engine(eng, cases["all"])
    assert np.array_equal(want[0], pods) and np.array_equal(want[1], st) and np.array_equal(want[3], res)


def test_min_member_partial(eng):
    ec, cases = DE.min_member_cases()
    c = cases["partial"]
    assert DE.min_member_cut_on_saturated_take(ec, c)
    want = MM.check_engine(eng, c)
    full, part, _, failed = MM.conditions(c.batch, c.min_member, want[1], want[2])
    assert full and part and failed


def test_gang_preempt(eng):
    inc, pc, who = DE.preempt_case()
    want = GP.check_engine(eng, pc)
    restored = DE.preempt_restores(inc, pc, want)
    for d in (DE.SMALL, DE.LARGE):
        assert any(kind == "kq" for _, dom, nodes in restored if dom == d for _, kind in nodes), restored
    assert (want[0] == -1).any() and (want[2] >= 1).any()
