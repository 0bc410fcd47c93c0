"""The edge cases of tests/decision_edges.py on the CPU: the three statements of the rule agree on them cell for
cell, the decision records show every line the cases are aimed at in both domain sizes, every wrong variant changes
an answer, and the other four calls' checkers agree with their Python statements on the edge pairs."""
import numpy as np
import pytest

import decision_edges as DE
import domain_placement as DP
import first_fit as FF
import gang_fit as GF
import gang_preempt as GP
import min_member as MM

_KW = {"key": "key", "take": "take", "island": "island_req", "back": "back"}


@pytest.fixture(scope="module")
def edge():
    """(EdgeCase, the C oracle's answer, place_python's, place_take_many's with the key variants watched)."""
    ec = DE.edge_case()
    args = DE.args_of(ec.case)
    return ec, DP.place(*args), DP.place_python(*args), DE.place_take_many(*args, watch=DE.KEYS)


def test_inventory_has_both_domain_sizes_and_every_edge_row():
    cap, used, labels, island, tag = DE.edge_inventory()
    res = cap - used
    for d, size in ((DE.SMALL, None), (DE.LARGE, DE.LDS + 1)):
        mine = island == d
        assert int(mine.sum()) == size if size else 64 < int(mine.sum()) < DE.LDS // 4
        assert (used[:, mine] > 0).any() and int(((res[:, mine] < 0).sum(axis=0) == 1).sum()) >= 4    # over-committed
        lines = {t for t, m in zip(tag, mine) if m and t is not None}
        assert set(DE.ARENAS) <= lines and {"S=SMAX-1", "S=SMAX", "r0=SMAX+1", "r2=2^20", "all INT64_MAX", "one -1"} <= lines
        assert len({int(x) for x in labels[mine]}) > len(DE.ARENAS)                                   # label bits differ
    assert not (island == DE.EMPTY).any() and (island == -1).any()


def test_three_statements_agree(edge):
    _, (pods, st, res), (p_pods, p_st, p_res, p_rb), (t_pods, t_st, t_res, t_rb, _, _) = edge
    assert st.tolist() == p_st == t_st
    assert pods.tolist() == p_pods == t_pods
    assert res.tolist() == p_res == t_res
    assert [(j, sorted(set(n))) for j, n in p_rb] == [(j, sorted(set(n))) for j, n in t_rb]


@pytest.mark.parametrize("domain", [DE.SMALL, DE.LARGE])
def test_every_line_is_shown(edge, domain):
    ec, _, _, answer = edge
    shown = DE.items_shown(ec, answer, domain)
    assert set(shown) == set(DE.ITEMS)
    missing = [item for item in DE.ITEMS if not shown[item]]
    assert missing == []


def test_empty_domain(edge):
    ec, (pods, st, _), _, _ = edge
    assert [int(st[j]) for n in ("empty_pod", "empty_none", "empty_island") for j in ec.jobs_named(n)] == [1, 0, 1]


@pytest.mark.parametrize("name", list(DE.VARIANTS))
def test_wrong_variant_changes_an_answer(edge, name):
    ec, _, _, right = edge
    wrong = DE.place_take_many(*DE.args_of(ec.case), **{_KW[k]: f for k, f in DE.VARIANTS[name].items()})
    changed = [d for d in (DE.SMALL, DE.LARGE) if DE.domain_answer(ec.case, wrong, d) != DE.domain_answer(ec.case, right, d)]
    print(name, "changes the answer in domains", changed)
    assert changed


def test_second_run_without_reset(edge):
    """The batch again on what the first run left: the statements still agree, and residuals sit elsewhere."""
    ec, (_, st, res), _, _ = edge
    args = DE.args_of(ec.case, res)
    a, b, c = DP.place(*args), DP.place_python(*args), DE.place_take_many(*args)
    assert a[1].tolist() == b[1] == c[1] and a[0].tolist() == b[0] == c[0] and a[2].tolist() == b[2] == c[2]
    assert a[1].tolist() != st.tolist()


def test_gang_fit_statements_agree(edge):
    ec = edge[0]
    c = ec.case
    pj, pd = DE.fit_pairs(ec)
    args = (c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)
    want, py = GF.answers(*args), GF.answers_python(*args)
    for w, p in zip(want, py):
        assert np.array_equal(w, p)
    assert set(pd.tolist()) == {DE.SMALL, DE.LARGE, DE.EMPTY} and (want[0] == 1).any() and (want[0] == 0).any()


@pytest.fixture(scope="module")
def first_fit():
    ec, pj, pd = DE.first_fit_case()
    c = ec.case
    args = (c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)
    return ec, pj, pd, FF.place_first_fit(*args), FF.place_first_fit_python(*args)


def test_first_fit_statements_agree(first_fit):
    _, _, _, want, py = first_fit
    for w, p in zip(want, py):
        assert np.array_equal(w, p)


def test_first_fit_crosses_for_an_edge_reason(first_fit):
    ec, pj, pd, (pods, st, pair, _), _ = first_fit
    assert DE.first_fit_crossed(ec, pj, pd, st, pair)
    j = ec.jobs_named("hopeless")[0]
    assert st[j] == 1 and pair[j] == -1


def test_min_member_statements_agree():
    ec, cases = DE.min_member_cases()
    got = {}
    for name, c in cases.items():
        args = (c.residual(), c.labels, c.island, c.batch, c.min_member, c.job_domain, c.level, c.level_size, c.parent)
        want, py = MM.place(*args), MM.place_python(*args)
        assert want[0].tolist() == py[0] and want[1].tolist() == py[1] and want[2].tolist() == py[2]
        assert want[3].tolist() == py[3]
        got[name] = want
    plain = DP.place(*DE.args_of(ec.case))
    for w, p in zip((got["all"][0], got["all"][1], got["all"][3]), plain):
        assert np.array_equal(w, p)
    assert DE.min_member_cut_on_saturated_take(ec, cases["partial"])
    full, part, none, failed = MM.conditions(cases["partial"].batch, cases["partial"].min_member, got["partial"][1], got["partial"][2])
    assert full and part and failed


@pytest.fixture(scope="module")
def preempt():
    inc, pc, who = DE.preempt_case()
    return inc, pc, who, pc.answers(), pc.answers(judge=GP.judge_python)


def test_preempt_statements_agree(preempt):
    _, _, _, want, py = preempt
    for w, p in zip(want, py):
        assert np.array_equal(w, p)


def test_preempt_release_restores_a_line(preempt):
    inc, pc, who, want, _ = preempt
    assert len(pc.vic) >= 20 and {"take_d1", "take_sat"} <= set(who)
    restored = DE.preempt_restores(inc, pc, want)
    print(restored)
    for d in (DE.SMALL, DE.LARGE):
        kinds = {k for _, dom, nodes in restored if dom == d for _, k in nodes}
        assert "kq" in kinds
    assert (want[0] == -1).any() and (want[2] >= 1).any()
