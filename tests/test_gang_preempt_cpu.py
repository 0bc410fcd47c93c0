"""pe_gang_preempt_domains on the CPU: the two instantiations of the two-phase procedure in tests/gang_preempt.py
agree on every named hierarchy and level, the hand-made traps give the values worked out by hand, the shared cases
show what they are meant to show, and the bindings match the header."""
import re

import numpy as np
import pytest

import domain_placement as DP
import gang_fit as GF
import gang_preempt as GP
import tree_capacity as TC
from placement import Engine, _abi

SIZES = (257, 1025)
TREE_LEVELS = [(name, n, level) for name in TC.TREES for n in SIZES for level in DP.tree_levels(name, n)]


@pytest.fixture(scope="module")
def cases():
    """The case and both instantiations' answers per (tree, n, level), computed once."""
    out = {}
    for name, n, level in TREE_LEVELS:
        pc = GP.tree_pcase(name, n, level)
        counts = []
        out[name, n, level] = (pc, pc.answers(counts=counts), pc.answers(judge=GP.judge_python), counts)
    return out


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_two_instantiations_agree(cases, name, n, level):
    _, oracle, python, _ = cases[name, n, level]
    for a, b in zip(oracle, python):
        assert a.tolist() == b.tolist()


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_cases_are_not_vacuous(cases, name, n, level):
    pc, (prefix, mask, count, best), _, counts = cases[name, n, level]
    lengths = np.diff(pc.pair_vic_off)
    assert {0, 1, 2, GP.MAX_LIST - 1, GP.MAX_LIST} <= set(lengths.tolist()), len(pc.vic)
    assert (prefix == 0).any()
    assert (prefix >= 1).any()
    assert (prefix == -1).any()
    assert ((count >= 0) & (count < prefix)).any()                               # a fill-back that fired
    # the outputs hang together, and the cost bound of the header holds pair by pair
    assert ((prefix == -1) == (count == -1)).all() and (mask[prefix <= 0] == 0).all()
    assert all(bin(int(m)).count("1") == c for m, c in zip(mask[count >= 0], count[count >= 0]))
    assert all(int(m) >> (int(k) - 1) == 1 for m, k in zip(mask[prefix >= 1], prefix[prefix >= 1]))   # position k - 1 stays
    assert all(made <= k + 1 + max(0, pre - 1) for made, k, pre in zip(counts, lengths.tolist(), prefix.tolist()))
    # the victims are accounted in `used`, with groups of several pods, island groups and pods in several domains
    c = pc.case
    assert (c.used >= 0).all() and len(pc.vic) >= 1
    # with empty lists the call is pe_gang_fit_domains: prefix 0 where it fits, best = first
    fits = GF.fits_oracle(c.residual(), c.labels, c.island, c.batch, pc.pair_job, pc.pair_domain, c.level, c.level_size,
                          c.parent)
    assert ((prefix == 0) == (fits == 1)).all()


@pytest.mark.parametrize("trap", sorted(GP.TRAPS))
def test_traps(trap):
    pc, want = GP.TRAPS[trap]()
    for judge in (GP.judge_oracle, GP.judge_python):
        got = pc.answers(judge=judge)
        assert [a.tolist() for a in got] == [list(w) for w in want]


def test_non_monotone_prefixes():
    """The prefixes of the header's example fit as no, yes, no: neither the full release nor a bisection is exact."""
    pc, _ = GP.trap_non_monotone()
    c = pc.case
    dom = DP.dom_level(c.island, 0, c.level_size, None)
    pods_of = [pc.vic.pods(v) for v in range(len(pc.vic))]
    fits = [GP.judge_python(GP.released(c.residual(), dom, 0, pods_of, [0, 1][:k]), c.labels, np.arange(2), GF.job_groups(c.batch, 0))
            for k in range(3)]
    assert fits == [False, True, False]


def test_empty_lists_are_gang_fit():
    pc = GP.tree_pcase("racks32", 257, 0)
    c = pc.case
    empty = np.zeros(len(pc.pair_job) + 1, dtype=np.int32)
    prefix, mask, count, best = GP.answers(c.residual(), c.labels, c.island, c.batch, pc.vic, pc.pair_job, pc.pair_domain, empty,
                                           np.zeros(0, dtype=np.int32), c.level, c.level_size, c.parent)
    fits = GF.fits_oracle(c.residual(), c.labels, c.island, c.batch, pc.pair_job, pc.pair_domain, c.level, c.level_size, c.parent)
    assert (prefix == np.where(fits == 1, 0, -1)).all() and not mask.any()
    assert best.tolist() == GF.first_of(pc.pair_job, fits, len(c.batch.job_group_off) - 1).tolist()


def test_bindings():
    sig = _abi.SIGNATURES["pe_gang_preempt_domains"]
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pe_gang_preempt_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "pe_gang_preempt_domains is not declared in placement.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig[1]) == 24
    P, i32, i64 = _abi.P, _abi.i32, _abi.i64
    for p, t in zip(params, sig[1]):
        want = P if "*" in p else i64 if p.startswith("int64_t") else i32
        assert t is want, (p, t)
    assert re.search(r"#define\s+PE_MAX_PAIR_VICTIMS\s+64\b", text) and _abi.PE_MAX_PAIR_VICTIMS == GP.MAX_LIST == 64
    assert callable(getattr(Engine, "gang_preempt_domains"))
    assert hasattr(_abi.load(), "pe_gang_preempt_domains")
