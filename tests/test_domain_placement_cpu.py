"""pe_place_greedy_domains on the CPU: the two statements of the rule in tests/domain_placement.py agree on
every named hierarchy and level, the shared cases show what they are meant to show, a hand-worked case, the
round trip with the capacity checker, and the bindings."""
import re

import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import gang_capacity as G
import tree_capacity as TC
import oracle
from placement import Engine, _abi, synth

SIZES = (257, 1025)
TREE_LEVELS = [(name, n, level) for name in TC.TREES for n in SIZES for level in DP.tree_levels(name, n)]


@pytest.fixture(scope="module")
def answers():
    """Both statements' answers per (tree, n, level), computed once."""
    out = {}
    for name, n, level in TREE_LEVELS:
        c = DP.tree_case(name, n, level)
        args = (c.residual(), c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent)
        out[name, n, level] = (c, DP.place(*args), DP.place_python(*args))
    return out


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_two_statements_agree(answers, name, n, level):
    _, (pods, st, res), (p_pods, p_st, p_res, _) = answers[name, n, level]
    assert st.tolist() == p_st
    assert pods.tolist() == p_pods
    assert res.tolist() == p_res


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_cases_are_not_vacuous(answers, name, n, level):
    c, (pods, st, _), (_, _, _, rollbacks) = answers[name, n, level]
    placed, failed, real_rollback, reused = DP.case_conditions(c.batch, c.job_domain, pods, st, rollbacks)
    b = c.batch
    groups = np.diff(b.job_group_off)
    assert (groups > 1).any() and (groups == 0).any()                           # multi-group jobs, a job without groups
    assert ((b.group_need & DP.ISLAND) != 0).any() and (b.group_count == 0).any()
    assert (b.group_req == 0).all(axis=1).any()                                 # a zero request
    assert len(set(b.priority.tolist())) < len(b.priority)                      # equal priorities
    per_domain = {}
    for d, p in zip(c.job_domain.tolist(), b.priority.tolist()):
        per_domain.setdefault(d, set()).add(p)
    assert any(len(v) > 1 for v in per_domain.values())                         # one domain, mixed priorities
    assert placed and failed
    # a rollback over two nodes needs a domain of two nodes: every level of every tree has one at these sizes
    # but the leaf level of "fanin" at 257 nodes (393 leaves, dealt round-robin: one node each)
    if DP.max_domain_nodes(c) >= 2:
        assert real_rollback and reused
    else:
        assert (name, n, level) == ("fanin", 257, 0)


def test_an_empty_domains_job_is_unschedulable():
    # "permuted" names twice as many leaves as it uses: the mix sends a job with pods and one without to an empty one
    c = DP.tree_case("permuted", 257, 0)
    dom = DP.dom_level(c.island, c.level, c.level_size, c.parent)
    pods, st, _ = DP.place(c.residual(), c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent)
    empty = [j for j, d in enumerate(c.job_domain) if not (dom == d).any()]
    assert len(empty) == 2
    has_pods = [int(c.batch.group_count[c.batch.job_group_off[j]:c.batch.job_group_off[j + 1]].sum()) > 0 for j in empty]
    assert sorted(has_pods) == [False, True]
    assert [int(st[j]) for j in empty] == [int(h) for h in has_pods]


def test_hand_worked_rack():
    """special_domains(): nodes 0 and 1 are rack 2, node 2 is rack 0.  For q = [2, 0, 1, 2] node 2 ([7, 0, 3, 9])
    has by far the smallest leftover and holds three pods (7 // 2, 3 // 1, 9 // 2 -> 3), so the unconstrained gang
    lands there.  Sent to rack 2, the gang sees nodes 0 and 1 only: node 0 ([5000, 8 GiB, 4, 100 GiB], score in the
    millions) beats node 1 (2^63 - 1 everywhere: the score saturates) and holds four pods (4 // 1), so three pods
    land on node 0 -- and of five, four on node 0 and the fifth on node 1."""
    cap, used, labels, island, n_domains = DC.special_domains()
    res = cap - used
    q = [2, 0, 1, 2]
    for count, want in ((3, [0, 0, 0]), (5, [0, 0, 0, 0, 1])):
        batch, dom = DP.make_batch([(2, 0, [(count, q, 0)])])
        for place in (DP.place, DP.place_python):
            pods, st, after = place(res, labels, island, batch, dom, 0, [n_domains], None)[:3]
            assert list(pods) == want and list(st) == [0]
            after = np.array(after, dtype=np.int64)
            assert after[:, 0].tolist() == (res[:, 0] - min(count, 4) * np.array(q)).tolist()
            assert after[:, 2].tolist() == res[:, 2].tolist()
    batch, _ = DP.make_batch([(2, 0, [(3, q, 0)])])
    pods, st, _ = oracle.place_greedy(res, labels, batch.job_group_off, batch.priority, batch.group_count,
                                      batch.group_req, batch.group_need)
    assert list(pods) == [2, 2, 2] and list(st) == [0]
    # rack 0 is node 2 alone: three pods fit, a fourth does not, and rack 1 has no node at all
    for d, count, want in ((0, 3, 0), (0, 4, 1), (1, 1, 1), (1, 0, 0)):
        batch, dom = DP.make_batch([(d, 0, [(count, q, 0)])])
        assert list(DP.place(res, labels, island, batch, dom, 0, [n_domains], None)[1]) == [want]


@pytest.mark.parametrize("name", TC.TREES)
def test_capacity_round_trip(name):
    """A one-group job sent to (level, domain) places exactly tree_slots[off_level + domain] pods, and not one more."""
    n = 257
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    res = cap - used
    shapes = [([16000, 64 * G.GiB, 0, 0], 0), ([8000, 32 * G.GiB, 2, 50 * G.GiB], 1)]
    req = np.array([q for q, _ in shapes], dtype=np.int64)
    need = np.array([nd for _, nd in shapes], dtype=np.uint32)
    slots, _ = TC.tables(res, labels, island, req, need, level_size, parent)
    off = TC.offsets(level_size)
    checked = 0
    for level in range(len(level_size)):
        for j, (q, nd) in enumerate(shapes):
            row = slots[j, off[level]:off[level + 1]]
            for d in sorted({int(row.argmax()), int(row.argmin()), 0, len(row) - 1}):
                s = int(row[d])
                for count, want in ((s, 0), (s + 1, 1)):
                    batch, dom = DP.make_batch([(d, 0, [(count, q, nd)])])
                    pods, st, after = DP.place(res, labels, island, batch, dom, level, level_size, parent)
                    assert list(st) == [want], (level, d, s, count)
                    if want:
                        assert np.array_equal(after, res) and (pods == -1).all()
                    else:
                        assert (pods >= 0).all()
                checked += 1
    assert checked >= 2 * len(level_size) and slots.max() > 0


def test_bindings():
    sig = _abi.SIGNATURES["pe_place_greedy_domains"]
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pe_place_greedy_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "pe_place_greedy_domains is not declared in placement.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig[1]) == 14
    P, i32, i64 = _abi.P, _abi.i32, _abi.i64
    for p, t in zip(params, sig[1]):
        want = P if "*" in p else i64 if p.startswith("int64_t") else i32
        assert t is want, (p, t)
    assert callable(getattr(Engine, "place_greedy_domains"))
