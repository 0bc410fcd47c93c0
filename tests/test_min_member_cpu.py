"""pe_place_min_member_domains on the CPU: the two statements of the rule in tests/min_member.py agree on every
named hierarchy and level, every mix shared with the GPU tests reaches both phases, the identities that follow
from the rule, the hand-made traps, and the bindings."""
import re

import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import gang_ledger as GL
import min_member as MM
import tree_capacity as TC
from placement import Engine, _abi, synth

SIZES = (257, 1025)
TREE_LEVELS = [(name, n, level) for name in TC.TREES for n in SIZES for level in DP.tree_levels(name, n)]
GPU_SIZES = (1, 255, 257, 1025, 2500)                 # test_gpu_place_min.py's trees
DOMAIN_SIZES = (1, 63, 64, 65, 255, 256, 257, 1015, 1016, 1017, 4097)


def args_of(c):
    return (c.residual(), c.labels, c.island, c.batch, c.min_member, c.job_domain, c.level, c.level_size, c.parent)


@pytest.fixture(scope="module")
def answers():
    """Both statements' answers per (tree, n, level), computed once."""
    out = {}
    for name, n, level in TREE_LEVELS:
        c = MM.tree_case(name, n, level)
        out[name, n, level] = (c, MM.place(*args_of(c)), MM.place_python(*args_of(c)))
    return out


@pytest.mark.parametrize("name,n,level", TREE_LEVELS)
def test_two_statements_agree(answers, name, n, level):
    _, (pods, st, gp, res), (p_pods, p_st, p_gp, p_res, _) = answers[name, n, level]
    assert st.tolist() == p_st
    assert gp.tolist() == p_gp
    assert pods.tolist() == p_pods
    assert res.tolist() == p_res


def test_min_member_draws_cover_the_kinds(answers):
    """0, 1, a group edge, inside a group, T - 1, T and -1 all occur in every tree's mixes (a level with one domain
    has too few jobs to show all seven by itself)."""
    for name in TC.TREES:
        kinds = set()
        for (tree, _, _), (c, _, _) in answers.items():
            if tree != name:
                continue
            jgo = c.batch.job_group_off
            for j, mm in enumerate(c.min_member.tolist()):
                cnt = [int(x) for x in c.batch.group_count[jgo[j]:jgo[j + 1]]]
                T, edges = sum(cnt), {sum(cnt[:k]) for k in range(1, len(cnt))}
                kinds |= {k for k, hit in (("0", mm == 0), ("1", mm == 1), ("T-1", mm == T - 1 and T > 1),
                                           ("T", mm == T and T > 0), ("all", mm == -1),
                                           ("edge", 0 < mm < T and mm in edges),
                                           ("inside", 0 < mm < T and mm not in edges)) if hit}
        assert kinds == {"0", "1", "T-1", "T", "all", "edge", "inside"}, (name, kinds)


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", GPU_SIZES)
def test_every_tree_mix_reaches_both_phases(name, n):
    """By the checker alone: a job placed in full, one placed in part, one placed with none of its optional pods
    and a failed one -- in every mix the CPU and the GPU tests use, so no case passes by never reaching phase 2."""
    for level in DP.tree_levels(name, n):
        c = MM.tree_case(name, n, level)
        _, st, gp, _ = MM.place(*args_of(c))
        assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True), (level,)


@pytest.mark.parametrize("size", DOMAIN_SIZES)
def test_every_size_case_reaches_both_phases(size):
    c = MM.size_case(size)
    pods, st, gp, res = MM.place(*args_of(c))
    assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True)
    assert st[2] == 1 and st[3] == 0 and gp[c.batch.job_group_off[4] + 1] == 3      # rolled back, reused, the island whole
    if size <= 257:
        p = MM.place_python(*args_of(c))
        assert (pods.tolist(), st.tolist(), gp.tolist(), res.tolist()) == p[:4]
        taken = set(p[4][0][1])                                                     # the nodes job 2 gave back
        poff = DP.pod_offsets(c.batch.group_count)
        g = int(c.batch.job_group_off[3])
        assert p[4][0][0] == 2 and taken & set(pods[poff[g]:poff[g + 1]].tolist())


def test_all_domains_active_mix_reaches_both_phases():
    c = MM.all_active_case()
    _, st, gp, _ = MM.place(*args_of(c))
    assert MM.conditions(c.batch, c.min_member, st, gp) == (True, True, True, True)
    assert len(set(c.job_domain.tolist())) == c.level_size[0]


# ---------------------------------------------------------------- identities

@pytest.mark.parametrize("name,n,level", [t for t in TREE_LEVELS if t[1] == 257])
def test_min_member_all_is_place_greedy_domains(answers, name, n, level):
    """min_member absent, -1 everywhere, or T_j everywhere: pods, statuses and residuals are domain_placement.place's."""
    c = answers[name, n, level][0]
    want = DP.place(c.residual(), c.labels, c.island, c.batch, c.job_domain, c.level, c.level_size, c.parent)
    _, _, _, T = MM.shares(c.batch, None)
    for mm in (None, np.full(len(T), -1, dtype=np.int32), np.array(T, dtype=np.int32)):
        a = list(args_of(c))
        a[4] = mm
        pods, st, gp, res = MM.place(*a)
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1]) and np.array_equal(res, want[2])
        jgo = c.batch.job_group_off
        for j in range(len(T)):
            assert gp[jgo[j]:jgo[j + 1]].tolist() == ([0] * (jgo[j + 1] - jgo[j]) if st[j] else
                                                      c.batch.group_count[jgo[j]:jgo[j + 1]].tolist())


@pytest.mark.parametrize("name", TC.TREES)
def test_min_member_zero_places_the_domains_slots(name):
    """M = 0 and one single-group job per domain: min(count, the domain's slots) pods are placed."""
    n = 257
    island, level_size, parent = TC.tree(name, n)
    cap, used, labels, island = DC.with_islands(synth.make_inventory(n, 23), island)
    res = cap - used
    off = TC.offsets(level_size)
    for q, nd in ((MM.Q, 0), (MM.Q_GPU, 1)):
        slots, _ = TC.tables(res, labels, island, np.array([q], dtype=np.int64), np.array([nd], dtype=np.uint32),
                             level_size, parent)
        for level in range(len(level_size)):
            row = slots[0, off[level]:off[level + 1]]
            count = max(1, int(np.median(row)))            # some domains hold it, some do not
            batch, dom, mm = MM.make_batch([(d, 0, 0, [(count, q, nd)]) for d in range(level_size[level])])
            pods, st, gp, _ = MM.place(res, labels, island, batch, mm, dom, level, level_size, parent)
            assert (st == 0).all() and gp.tolist() == np.minimum(row, count).tolist()
            if level == 0:
                leaf, _ = DC.tables(res, labels, island, np.array([q], dtype=np.int64), np.array([nd], dtype=np.uint32),
                                    level_size[0])
                assert gp.tolist() == np.minimum(leaf[0], count).tolist()


@pytest.mark.parametrize("name,n,level", [t for t in TREE_LEVELS if t[1] == 257])
def test_release_restores_the_residuals(answers, name, n, level):
    """The outputs go straight to the ledger: releasing them gives the residuals before the call, bit for bit."""
    c, (pods, st, gp, res), _ = answers[name, n, level]
    out = GL.release(res, c.residual(), np.zeros(res.shape[1], dtype=bool), GL.of_batch(c.batch, pods))
    assert out.node == -1 and out.pods == int(gp.sum()) and np.array_equal(out.res, c.residual())


# ---------------------------------------------------------------- traps

@pytest.mark.parametrize("trap", sorted(MM.traps()))
def test_traps(trap):
    c, want_st, want_gp = MM.traps()[trap]
    o = MM.place(*args_of(c))
    p = MM.place_python(*args_of(c))
    assert (o[0].tolist(), o[1].tolist(), o[2].tolist(), o[3].tolist()) == p[:4]
    assert o[1].tolist() == want_st and o[2].tolist() == want_gp
    poff = DP.pod_offsets(c.batch.group_count)
    for g, k in enumerate(want_gp):                        # within a group the placed slots are a prefix
        assert (o[0][poff[g]:poff[g] + k] >= 0).all() and (o[0][poff[g] + k:poff[g + 1]] == -1).all()


def test_the_rack_of_the_header():
    c, _, _ = MM.traps()["rack_min4"]
    pods, st, gp, res = MM.place(*args_of(c))
    assert st.tolist() == [0] and gp.tolist() == [1, 4] and pods[5:].tolist() == [-1, -1] and (pods[:5] >= 0).all()
    assert sorted(res[2].tolist()) == [0, 2]
    b = c.batch
    assert DP.place(c.residual(), c.labels, c.island, b, c.job_domain, 0, [1], None)[1].tolist() == [1]
    c6, _, _ = MM.traps()["rack_min6"]
    pods, st, gp, res = MM.place(*args_of(c6))
    assert st.tolist() == [1] and (pods == -1).all() and np.array_equal(res, c6.residual())


# ---------------------------------------------------------------- the bindings

def test_bindings():
    sig = _abi.SIGNATURES["pe_place_min_member_domains"]
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+pe_place_min_member_domains\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, "pe_place_min_member_domains is not declared in placement.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig[1]) == 17
    P, i32, i64 = _abi.P, _abi.i32, _abi.i64
    for p, t in zip(params, sig[1]):
        want = P if "*" in p else i64 if p.startswith("int64_t") else i32
        assert t is want, (p, t)
    assert re.search(r"#define\s+PE_MIN_MEMBER_ALL\s+\(-1\)", text)
    assert hasattr(_abi.load(), "pe_place_min_member_domains")


def test_binding_argument_checks():
    """Shapes the binding refuses before the library is called (no engine needed: the checks come first)."""
    e = Engine.__new__(Engine)
    call = Engine.place_min_member_domains
    base = dict(job_group_off=[0, 1, 2], priority=[0, 0], group_count=[1, 1], group_req=[MM.ONE, MM.ONE], group_need=None,
                min_member=[1, 1], job_domain=[0, 0], level=0, level_size=[1])
    for key, bad in (("min_member", [1]), ("min_member", [[1, 1]]), ("job_domain", [0]), ("level_size", None)):
        with pytest.raises(ValueError):
            call(e, **{**base, key: bad})
