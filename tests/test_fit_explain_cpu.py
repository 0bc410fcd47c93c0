"""The checker of pe_fit_explain (tests/fit_explain.py) against itself, the C oracle and the rule's worked example;
what the shared inputs reach; and the bindings.  No GPU."""
import os
import re

import numpy as np
import pytest

import fit_explain as X
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return X.threshold_cases() + [X.arena(), X.near_edges(), X.worked_example()]


@pytest.fixture(scope="module")
def answers(cases):
    return {c.name: X.explain(*c.reference(), c.req, c.need) for c in cases}


def test_the_two_statements_agree(cases, answers):
    for c in cases:
        res, lab = c.reference()
        J = len(c.req)
        pick = np.arange(J) if J <= 12 else np.unique(np.linspace(0, J - 1, 12).astype(int))   # cell by cell is slow
        hist, near = X.explain_cells(res, lab, c.req[pick], c.need[pick])
        np.testing.assert_array_equal(hist, answers[c.name][0][pick], err_msg=c.name)
        np.testing.assert_array_equal(near, answers[c.name][1][pick], err_msg=c.name)


def test_the_two_statements_agree_on_domains():
    case, level_size, parent = X.tree_case("orphans", 257)
    res, lab = case.reference()
    for level in range(len(level_size)):
        dom = X.level_domains(case.island, level_size, parent, level)
        jd = (np.arange(8) % (level_size[level] + 1) - 1).astype(np.int32)     # ANY and every small id
        a = X.explain_cells(res, lab, case.req[:8], case.need[:8], dom, jd)
        b = X.explain(res, lab, case.req[:8], case.need[:8], dom, jd)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert (jd == X.ANY).any() and (dom == X.NO_DOMAIN).any()


def test_bin_zero_is_the_oracles_fit_count_and_rows_sum_to_the_live_nodes(cases, answers):
    for c in cases:
        res, lab = c.reference()
        _, counts = oracle.fit_mask(res, lab, c.req, c.need)
        hist = answers[c.name][0]
        np.testing.assert_array_equal(hist[:, 0], counts, err_msg=c.name)
        assert (hist.sum(axis=1) == len(lab) - len(c.remove)).all(), c.name
        assert (hist >= 0).all()


def test_coverage(cases, answers):
    """Computed by the checker alone: every bin and every near dimension is reached, with the edge values."""
    hist = np.concatenate([answers[c.name][0] for c in cases])
    near = np.concatenate([answers[c.name][1] for c in cases])
    assert (hist > 0).any(axis=0).all(), np.flatnonzero(~(hist > 0).any(axis=0))
    assert (near > 0).any(axis=0).all()
    assert (answers["arena"][0] == 1)[0, 1:].all() and answers["arena"][0][0, 0] == 1025 - 31
    assert answers["arena"][1].tolist() == [[1, 2, 3, 4]]
    edge = {int(v) for v in answers["near"][1].reshape(-1)}
    assert {1, 1 << 63, (1 << 64) - 2} <= edge, edge
    # the tie: two nodes at the minimum
    res, _ = X.near_edges().reference()
    assert (res[2] == 4).sum() == 2 and int(answers["near"][1][3, 2]) == 1


@pytest.mark.parametrize("variant", X.VARIANTS)
def test_every_wrong_variant_changes_some_cell(variant, cases, answers):
    """A condition on the inputs: adjust them, not the variants."""
    changed = []
    for c in cases:
        res, lab = c.reference()
        got = X.explain(res, lab, c.req, c.need, variants=(variant,), island=c.island)
        if (got[0] != answers[c.name][0]).any() or (got[1] != answers[c.name][1]).any():
            changed.append(c.name)
    if variant == "level0":      # the domain form: the same nodes, the domain of level 1 against level 0
        case, level_size, parent = X.tree_case("racks32", 257)
        res, lab = case.reference()
        dom = [X.level_domains(case.island, level_size, parent, l) for l in (0, 1)]
        jd = (np.arange(len(case.req)) % level_size[1]).astype(np.int32)
        want = X.explain(res, lab, case.req, case.need, dom[1], jd)
        got = X.explain(res, lab, case.req, case.need, dom[1], jd, variants=(variant,), dom0=dom[0])
        if (got[0] != want[0]).any() or (got[1] != want[1]).any():
            changed.append(case.name)
    assert changed, variant


def test_worked_example_and_message(answers):
    hist, near = answers["example"]
    want = np.zeros(X.BINS, dtype=np.int64)
    for s, c in X.EXAMPLE_HIST.items():
        want[s] = c
    np.testing.assert_array_equal(hist[0], want)
    assert near[0].tolist() == list(X.EXAMPLE_NEAR) and hist[0].sum() == 5
    assert X.message(hist[0]) == X.EXAMPLE_MESSAGE
    assert X.message([7] + [0] * 31) == "7/7 nodes are available."
    from placement import FitExplain, explain_message
    assert explain_message(hist[0]) == X.EXAMPLE_MESSAGE and explain_message([7] + [0] * 31) == "7/7 nodes are available."
    fx = FitExplain(hist, near)
    assert fx.message(0) == X.EXAMPLE_MESSAGE and fx.fits.tolist() == [1] and fx.live.tolist() == [5]
    assert fx.insufficient.tolist() == [[1, 1, 3, 0]] and fx.label_mismatch.tolist() == [1]
    assert fx.only.tolist() == [[0, 0, 2, 0]]
    assert fx.message(0, ("a", "b", "c", "d")).count("Insufficient c") == 1


def test_messages_of_every_case_match_the_binding(cases, answers):
    from placement import explain_message
    for c in cases:
        for row in answers[c.name][0][:20]:
            assert explain_message(row) == X.message(row)


def test_weighted_form_equals_the_plain_checker():
    case = X.threshold_cases()[1]
    res, lab = case.reference()
    keep = np.flatnonzero(res[0] != X.NEVER)[:100]
    rows, labels, weight = X.tiled(res[:, keep].T, lab[keep], 1500, 3)
    plain = X.explain(rows.T, labels, case.req, case.need)
    weighted = X.explain(res[:, keep], lab[keep], case.req, case.need, weight=weight)
    np.testing.assert_array_equal(plain[0], weighted[0])
    np.testing.assert_array_equal(plain[1], weighted[1])
    assert weight.sum() == 1500 and weight.min() >= 1


def test_abi_table_library_and_engine_have_the_call():
    from placement import Engine, _abi
    assert "pe_fit_explain" in _abi.SIGNATURES and len(_abi.SIGNATURES["pe_fit_explain"][1]) == 11
    assert hasattr(_abi.load(), "pe_fit_explain")
    assert callable(getattr(Engine, "fit_explain"))


def test_go_binds_the_call_and_defines_message():
    with open(os.path.join(ROOT, "go", "pkg", "placement", "hip", "hip.go")) as f:
        go = f.read()
    call = re.search(r"C\.pe_fit_explain\(([^\n]*)\)\n", go)
    assert call and len(call.group(1).split(", ")) == 11
    assert re.search(r"func \(e \*Engine\) FitExplain\(", go)
    assert re.search(r"func \(x \*FitExplanation\) Message\(", go)
    assert "didn't match the required labels" in go
