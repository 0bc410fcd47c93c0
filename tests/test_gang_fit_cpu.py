"""pe_gang_fit_domains on the CPU: the two statements of the rule in tests/gang_fit.py agree on every named
hierarchy and level, the shared cases show what they are meant to show, the header's two-node example by hand, the
round trip with the capacity checker, and the bindings."""
import re

import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import gang_capacity as G
import gang_fit as GF
import tree_capacity as TC
from placement import Engine, _abi, synth

SIZES = (257, 1025)
TREE_LEVELS = [(name, n, level) for name in TC.TREES for n in SIZES for level in DP.tree_levels(name, n)]
ALL_OR_NOTHING = {("four", 1025, 2), ("permuted", 257, 2), ("permuted", 1025, 2)}


@pytest.fixture(scope="module")
def cases():
    """The case, its pairs and both statements' answers per (tree, n, level), computed once."""
    out = {}
    for name, n, level in TREE_LEVELS:
        c, pj, pd = GF.pairs_case(name, n, level)
        args = (c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)
        out[name, n, level] = (c, pj, pd, GF.answers(*args), GF.answers_python(*args))
    return out


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_two_statements_agree(cases, name, n, level):
    c, pj, pd, (fits, fail, pods), (p_fits, p_fail, p_pods) = cases[name, n, level]
    assert fits.tolist() == p_fits.tolist()
    assert fail.tolist() == p_fail.tolist() and pods.tolist() == p_pods.tolist()     # the oracle's walk and bisection too
    assert fits.tolist() == GF.fits_oracle(c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size,
                                           c.parent).tolist()


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_cases_are_not_vacuous(cases, name, n, level):
    c, pj, pd, (fits, fail, pods), _ = cases[name, n, level]
    J = len(c.batch.job_group_off) - 1
    first = GF.first_of(pj, fits, J)
    assert not (np.diff(pj) >= 0).all()                                          # not grouped by job
    assert len(set(zip(pj.tolist(), pd.tolist()))) < len(pj)                     # pairs repeat
    assert fits.any()
    # a job that takes pods and then fails needs a domain of two usable nodes: every level of every tree has one at
    # these sizes but the leaf level of "fanin" at 257 nodes (393 leaves, dealt round-robin: one node each)
    partial = ((fits == 0) & (fail > 0) & (pods > 0)).any()
    if DP.max_domain_nodes(c) >= 2:
        assert partial
    else:
        assert (name, n, level) == ("fanin", 257, 0)
    # a job whose first pair does not fit and a later one does needs two domains that differ for it: every level of
    # more than one domain shows one, but the three in ALL_OR_NOTHING -- two or three domains of hundreds of nodes
    # each, in which every job of the mix that fits one domain fits them all
    first_pair = GF.first_of(pj, np.ones_like(fits), J)
    later = bool(((first >= 0) & (first != first_pair)).any())
    assert later == (c.level_size[c.level] > 1 and (name, n, level) not in ALL_OR_NOTHING), (name, n, level)


def test_oracle_statement_is_domain_placements():
    """fits_oracle's step for one job is domain_placement.place with that job alone, pair by pair."""
    c, pj, pd = GF.pairs_case("permuted", 257, 1)
    fits = GF.fits_oracle(c.residual(), c.labels, c.island, c.batch, pj, pd, c.level, c.level_size, c.parent)
    assert fits.any() and not fits.all()
    for p in range(0, len(pj), 3):
        batch, dom = DP.make_batch([(int(pd[p]), 0, GF.job_groups(c.batch, int(pj[p])))])
        _, st, _ = DP.place(c.residual(), c.labels, c.island, batch, dom, c.level, c.level_size, c.parent)
        assert int(st[0]) == 1 - int(fits[p])


def two_node_rack():
    """A rack of two nodes with 8 free GPUs each (cpu and memory to spare), and a rack without nodes."""
    res = np.array([[64000, 64000], [256 * G.GiB, 256 * G.GiB], [8, 8], [0, 0]], dtype=np.int64)
    island = np.array([0, 0], dtype=np.int32)
    labels = synth.island_labels(np.array([1, 1], dtype=np.uint32), island)
    return res, labels, island


def test_hand_worked_two_nodes():
    """include/placement.h's example.  A = 2 pods x 5 GPUs, B = 3 pods x 2 GPUs: MinResources 16 <= 16, A's slots 2,
    B's slots 8 -- but A takes one node each, 3 + 3 GPUs are left, and B places two of its three pods: fits 0,
    fail_group 1, pods 2 + 2.  With B's count 2 the gang fits: pods 4."""
    res, labels, island = two_node_rack()
    a, b3, b2 = (2, [1000, G.GiB, 5, 0], 0), (3, [1000, G.GiB, 2, 0], 0), (2, [1000, G.GiB, 2, 0], 0)
    batch, _ = DP.make_batch([(0, 0, [a, b3]), (0, 0, [a, b2]), (0, 0, [b3, a])])
    pj, pd = np.array([0, 1, 2, 0], dtype=np.int32), np.array([0, 0, 0, 1], dtype=np.int32)
    for statement in (GF.answers, GF.answers_python):
        fits, fail, pods = statement(res, labels, island, batch, pj, pd, 0, [2], None)
        assert fits.tolist() == [0, 1, 0, 0]
        assert fail.tolist() == [1, -1, 1, 0]          # B first: 3 x 2 on one node (best fit), then A finds one node of 8
        assert pods.tolist() == [4, 4, 4, 0]
    assert GF.first_of(pj, fits, 3).tolist() == [-1, 1, -1]
    # every read-only call we had says yes: the slots of each group alone
    slots, _ = TC.tables(res, labels, island, np.array([a[1], b3[1]], dtype=np.int64), np.zeros(2, dtype=np.uint32), [2], None)
    assert slots[:, 0].tolist() == [2, 8] and 2 * 5 + 3 * 2 <= int(res[2].sum())


@pytest.mark.parametrize("name", TC.TREES)
def test_one_group_is_the_capacity(name):
    """A one-group job without an island need fits (level, domain) iff tree_slots[off_level + domain] >= count."""
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
        jobs, pj, pd, want = [], [], [], []
        for s, (q, nd) in enumerate(shapes):
            row = slots[s, off[level]:off[level + 1]]
            for d in sorted({int(row.argmax()), int(row.argmin()), 0, len(row) - 1}):
                for count in (int(row[d]), int(row[d]) + 1, max(1, int(row[d]) // 2)):
                    pj.append(len(jobs))
                    pd.append(d)
                    want.append(int(int(row[d]) >= count))
                    jobs.append((d, 0, [(count, q, nd)]))
        batch, _ = DP.make_batch(jobs)
        fits, fail, pods = GF.answers(res, labels, island, batch, np.array(pj), np.array(pd), level, level_size, parent)
        assert fits.tolist() == want
        assert all(f == (-1 if w else 0) for f, w in zip(fail.tolist(), want))
        checked += len(want)
    assert checked >= 6 * len(level_size) and slots.max() > 0


def test_bindings():
    sig = _abi.SIGNATURES["pe_gang_fit_domains"]
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pe_gang_fit_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "pe_gang_fit_domains is not declared in placement.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig[1]) == 17
    P, i32, i64 = _abi.P, _abi.i32, _abi.i64
    for p, t in zip(params, sig[1]):
        want = P if "*" in p else i64 if p.startswith("int64_t") else i32
        assert t is want, (p, t)
    assert callable(getattr(Engine, "gang_fit_domains"))
