"""pe_drain_fit_domains on the CPU: the checker's two statements of the rule (tests/drain_fit.py) agree on every named
hierarchy x every level at N = 257 and 1025 and on the hand-made traps; every wrong reading of the rule changes at
least one cell on these inputs; every case shows what it is there to show; and the binding agrees with the header."""
import functools
import os
import re

import numpy as np
import pytest

import domain_placement as DP
import drain_fit as DF
import tree_capacity as TC
from oracle import semantics as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(name, n, level) for name in TC.TREES for n in (257, 1025) for level in DP.tree_levels(name, n)]


@functools.lru_cache(maxsize=None)
def tree_case(name, n, level):
    dc = DF.tree_drain_case(name, n, level)
    return dc, DF.drain_python(*dc.checker_args())


@pytest.mark.parametrize("name,n,level", CASES)
def test_statements_agree_on_named_trees(name, n, level):
    dc, py = tree_case(name, n, level)
    want = DF.drain_oracle(*dc.checker_args())
    for a, b, what in zip(py, want, ("fits", "moved", "fail_slot", "target")):
        assert np.array_equal(a, b), (what, np.nonzero(a != b)[0][:10].tolist())


@pytest.mark.parametrize("trap", sorted(DF.traps()))
def test_statements_agree_on_traps(trap):
    dc, expected = DF.traps()[trap]
    py = DF.drain_python(*dc.checker_args())
    assert DF.same(py, DF.drain_oracle(*dc.checker_args()))
    if expected is not None:
        assert [x.tolist() for x in py] == [list(x) for x in expected]


def test_worked_example_by_fit_python():
    """The header's example, by the fit call's own Python statement on the rack without A."""
    import gang_fit as GF
    dc, _ = DF.traps()["worked_fails"]
    two, three = (2, DF.gpus(2), 0), (1, DF.gpus(3), 0)
    assert GF.fit_python(dc.res, dc.case.labels, [1, 2], [two, three]) == (0, 1, 2)
    assert GF.fit_python(dc.res, dc.case.labels, [1, 2], [three, two]) == (1, -1, 3)


def test_every_variant_changes_a_cell():
    """On the inputs the GPU test uses: the traps and the named trees at N = 257."""
    inputs = [dc for dc, _ in DF.traps().values()] + [tree_case(name, 257, level)[0] for name, n, level in CASES if n == 257]
    right = [DF.drain_python(*dc.checker_args()) for dc in inputs]
    for variant in DF.VARIANTS:
        changed = sum(not DF.same(DF.drain_python(*dc.checker_args(), variant=variant), r) for dc, r in zip(inputs, right))
        assert changed > 0, variant


def conditions(dc, ans):
    """What a case shows, by the checker alone: (a candidate with pods that fits, one that fails with moved > 0, one
    whose excluded node would have been an argmin, one whose target domain is not its node's own, one with an island
    run, one with pods of two gangs)."""
    fits, moved, _, target = ans
    book, c = dc.book, dc.case
    dom = DP.dom_level(c.island, c.level, c.level_size, c.parent)
    group_of = book.group_of_slot()
    gang_of = np.repeat(np.arange(len(book.off) - 1), np.diff(book.off))[group_of]
    live = [k for k, n in enumerate(dc.cand_node) if not DF.removed(dc.res, int(n))]
    on = {k: np.nonzero(book.pod == dc.cand_node[k])[0] for k in live}

    def own_best(k):
        """Whether the candidate's node, were it kept, would be the argmin of its own first pod."""
        n, g = int(dc.cand_node[k]), group_of[on[k][0]] if len(on[k]) else -1
        if g < 0 or book.need[g] & DF.ISLAND:
            return False
        keys = [S.appendix_b_key([int(dc.res[d][i]) for d in range(4)], int(c.labels[i]), [int(x) for x in book.req[g]],
                                 int(book.need[g]), int(i)) for i in np.nonzero(dom == dc.cand_domain[k])[0]]
        return min((x for x in keys if x is not None), default=-1) & 0xFFFFFF == n

    return (any(fits[k] and moved[k] > 0 for k in live),
            any(not fits[k] and moved[k] > 0 for k in live),
            any(own_best(k) for k in live),
            any(len(on[k]) and dom[dc.cand_node[k]] != dc.cand_domain[k] for k in live),
            any(((book.need[group_of[on[k]]] & DF.ISLAND) != 0).any() for k in live),
            any(len(set(gang_of[on[k]])) >= 2 for k in live))


SHOWN = ("fits", "fails with moved > 0", "excluded argmin", "foreign domain", "island run", "two gangs")
# the cases that do not show everything, by name: what each lacks
ONE_DOMAIN = ("foreign domain",)      # the level has one populated domain: there is no other to drain into
EXCEPTIONS = {("racks32", 257, 2): ONE_DOMAIN, ("racks32", 1025, 2): ONE_DOMAIN, ("four", 257, 3): ONE_DOMAIN,
              ("four", 1025, 3): ONE_DOMAIN, ("orphans", 257, 2): ONE_DOMAIN, ("orphans", 1025, 2): ONE_DOMAIN,
              ("fanin", 257, 2): ONE_DOMAIN, ("fanin", 1025, 2): ONE_DOMAIN}


@pytest.mark.parametrize("name,n,level", CASES)
def test_cases_show_what_they_are_for(name, n, level):
    dc, py = tree_case(name, n, level)
    lacking = tuple(s for s, ok in zip(SHOWN, conditions(dc, py)) if not ok)
    assert lacking == EXCEPTIONS.get((name, n, level), ()), lacking
    if lacking == ONE_DOMAIN:
        dom = DP.dom_level(dc.case.island, level, dc.case.level_size, dc.case.parent)
        assert len(np.unique(dom[dom >= 0])) == 1
    assert dc.gone and dc.gone[0] in dc.cand_node.tolist()      # a candidate on a removed slot, with pods
    assert (dc.book.pod == dc.gone[0]).any()


def test_binding_agrees_with_header():
    from placement import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "placement.h")).read(), flags=re.S)
    m = re.search(r"\bint pe_drain_fit_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _abi.SIGNATURES["pe_drain_fit_domains"]
    assert len(params) == len(args) == 18
    for p, a in zip(params, args):
        want = _abi.P if "*" in p else _abi.i64 if p.startswith("int64_t") else _abi.i32
        assert a is want, (p, a)
    go = open(os.path.join(ROOT, "go", "pkg", "placement", "hip", "hip.go")).read()
    assert "func (e *Engine) DrainFitDomains(" in go and "C.pe_drain_fit_domains(" in go
