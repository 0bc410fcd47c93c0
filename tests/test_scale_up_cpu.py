"""pe_scale_up_domains on the CPU: the checker's two statements of the rule (tests/scale_up.py) agree on every named
hierarchy x every level at N = 257 and 1025 and on the hand-made traps; every wrong reading of the rule changes at
least one cell on these inputs; every trap listed as non-monotone is, in both statements; every case shows what it
is there to show; with pair_max 0 the call is pe_gang_fit_domains; and the binding agrees with the header."""
import functools
import os
import re

import numpy as np
import pytest

import domain_placement as DP
import gang_fit as GF
import scale_up as SU
import tree_capacity as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(name, n, level) for name in TC.TREES for n in (257, 1025) for level in DP.tree_levels(name, n)]


@functools.lru_cache(maxsize=None)
def tree_case(name, n, level):
    sc = SU.tree_scale_case(name, n, level)
    return sc, SU.scale_python(sc)


@pytest.mark.parametrize("name,n,level", CASES)
def test_statements_agree_on_named_trees(name, n, level):
    sc, py = tree_case(name, n, level)
    for a, b, what in zip(py, SU.scale_oracle(sc), SU.NAMES):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, np.nonzero(a != b)[0][:10].tolist())


@pytest.mark.parametrize("trap", sorted(SU.traps()))
def test_statements_agree_on_traps(trap):
    sc, expected = SU.traps()[trap]
    py = SU.scale_python(sc)
    assert SU.same(py, SU.scale_oracle(sc))
    for got, want, what in zip(py, expected, SU.NAMES):
        if want is not None:
            assert got.tolist() == list(want), what


@pytest.mark.parametrize("trap", sorted(SU.NON_MONOTONE))
def test_non_monotone_traps_are(trap):
    """There is a k that fits and a larger k <= K that does not, by the Python statement and by the C oracle; and
    the k that fit are the listed ones."""
    sc, _ = SU.traps()[trap]
    free, _, _, K, fit_ks = SU.NON_MONOTONE[trap]
    nodes = np.arange(len(free))
    groups = GF.job_groups(sc.case.batch, 0)
    by_oracle = [k for k in range(K + 1) if SU.attempt_oracle(sc, nodes, groups, 0, k)[0]]
    by_python = [k for k in range(K + 1) if SU.attempt_python(sc, nodes, groups, 0, k)[0]]
    assert by_oracle == by_python == fit_ks
    assert any(k not in fit_ks for k in range(fit_ks[0], K + 1))


def test_every_variant_changes_a_cell():
    """On the inputs the GPU test uses: the traps and the named trees at N = 257."""
    inputs = [sc for sc, _ in SU.traps().values()] + [tree_case(name, 257, level)[0] for name, n, level in CASES if n == 257]
    right = [SU.scale_python(sc) for sc in inputs]
    for variant in SU.VARIANTS:
        changed = sum(not SU.same(SU.scale_python(sc, variant=variant), r) for sc, r in zip(inputs, right))
        assert changed > 0, variant


@pytest.mark.parametrize("name,n,level", CASES)
def test_cases_show_what_they_are_for(name, n, level):
    """A pair answered 0, one answered >= 2, one answered -1, and a job whose best pair is not its first; removed
    slots below, between and above the live ids; new slots among them."""
    sc, (nodes, _, _, new_pods, best) = tree_case(name, n, level)
    assert (nodes == 0).any() and (nodes >= 2).any() and (nodes == -1).any()
    first = GF.first_of(sc.pair_job, np.ones(len(sc.pair_job), dtype=bool), len(best))
    assert ((best >= 0) & (best != first)).any()
    assert (new_pods > 0).any()
    live = np.nonzero(sc.res[0] != SU.NEVER)[0]
    gone = np.array(sc.gone)
    assert (gone < live.min()).any() and (gone > live.max()).any() and ((gone > live.min()) & (gone < live.max())).any()
    assert set(sc.new_slot.tolist()) <= set(sc.gone) and len(set(sc.new_slot.tolist())) == len(sc.new_slot)


@pytest.mark.parametrize("name,n,level", [c for c in CASES if c[1] == 257])
def test_pair_max_zero_is_gang_fit(name, n, level):
    """With every K_p = 0: out_nodes = out_fits - 1, fail_group and pods are pe_gang_fit_domains', new_pods is 0 and
    out_best is out_first."""
    sc, _ = tree_case(name, n, level)
    zero = SU.ScaleCase(sc.case, sc.res, sc.gone, sc.tmpl_res, sc.tmpl_labels, sc.new_slot, sc.pair_job, sc.pair_domain,
                        sc.pair_template, np.zeros(len(sc.pair_job), dtype=np.int32))
    c = sc.case
    island = np.where(sc.res[0] == SU.NEVER, -1, c.island)           # a removed slot is in no domain
    fits, fail, pods = GF.answers(sc.res, c.labels, island, c.batch, sc.pair_job, sc.pair_domain, c.level, c.level_size, c.parent)
    for ans in (SU.scale_oracle(zero), SU.scale_python(zero)):
        assert np.array_equal(ans[0], fits.astype(np.int32) - 1)
        assert np.array_equal(ans[1], fail) and np.array_equal(ans[2], pods) and not ans[3].any()
        assert np.array_equal(ans[4], GF.first_of(sc.pair_job, fits, len(ans[4])))


def test_binding_agrees_with_header():
    from placement import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "placement.h")).read(), flags=re.S)
    m = re.search(r"\bint pe_scale_up_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _abi.SIGNATURES["pe_scale_up_domains"]
    assert len(params) == len(args) == 25
    for p, a in zip(params, args):
        want = _abi.P if "*" in p else _abi.i64 if p.startswith("int64_t") else _abi.i32
        assert a is want, (p, a)
    assert _abi.PE_MAX_SCALE_NODES == int(re.search(r"#define PE_MAX_SCALE_NODES (\d+)", text).group(1)) == 64
    assert hasattr(_abi.load(), "pe_scale_up_domains")
    go = open(os.path.join(ROOT, "go", "pkg", "placement", "hip", "hip.go")).read()
    assert "func (e *Engine) ScaleUpDomains(" in go and "C.pe_scale_up_domains(" in go
