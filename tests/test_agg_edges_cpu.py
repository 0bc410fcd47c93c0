"""The int64 edge cases of the aggregation (tests/agg_edges.py) before any GPU run: the big-integer checker
(tests/wide_agg.py) and the C oracle agree on every variant batch, every hand-worked value is the checker's,
every step of agg_job_t has a job on each side of int64 in every variant that can reach it, the variants
are packed the way they claim, and every fault of agg_edges.FAULTS changes some job's answer.  No GPU."""
import numpy as np
import pytest

import agg_edges as E
import oracle
import wide_agg as WA
from wide_agg import V1, V2

VARIANTS = [None] + list(E.SHIFTS)            # None: the unnarrowable variant; else the edge key's shift
IDS = ["wide"] + [f"s{s}" for s in E.SHIFTS]


def variant_batch(mode, v):
    """Two keys: the edge in key 0 on shift v, key 1 with ordinary values on another shift."""
    sh = None if v is None else [v, 0 if v == 1 else 1]
    arrs, cases = E.edge_batch(mode, 2, sh, edge_keys=[0])
    return arrs, cases, sh


def checker(mode, arrs, n_keys):
    return WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], n_keys)


@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_references_agree_and_hand_values_hold(mode, v):
    """Checker == C oracle on flags, presence, members and the values of unflagged jobs; every case's value,
    flag, presence and members as worked out by hand; no job reaches flag 2; the restated rule (the copy
    that records the steps) is the checker, from the caller's cells and from the packed ones."""
    arrs, cases, sh = variant_batch(mode, v)
    vals, pres, mem, flag = checker(mode, arrs, 2)
    o_vals, o_pres, o_mem, o_ovf = oracle.pg_min_resources_keys(mode, *arrs)
    assert not (flag == 2).any()
    np.testing.assert_array_equal(flag, o_ovf)
    np.testing.assert_array_equal(pres, o_pres)
    np.testing.assert_array_equal(mem, o_mem)
    ok = flag == 0
    np.testing.assert_array_equal(vals[ok], o_vals[ok].astype(object))
    assert not o_vals[~ok].any()                            # a flagged key zeroes the job's other keys too
    for j, c in enumerate(cases):
        assert flag[j] == c["flag"], c["name"]
        assert vals[j, 0] == c["want"], (c["name"], vals[j, 0])
        assert bool(pres[j] & 1) == c["pres"], c["name"]
        assert mem[j] == c["mem"], (c["name"], mem[j])
        if c["pres"]:
            assert pres[j] & 2, c["name"]                   # the other key is present beside the edge
    want = E.int64_answers((vals, pres, mem, flag))
    for pack in (False, True) if sh is not None else (False,):
        assert E.same_answers(E.model(mode, *arrs, 2, pack=pack), want).all(), pack


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_every_step_has_both_sides(v):
    """Coverage asserted, not assumed: for each step with an overflow test that the variant's grid can
    reach, a flag-0 job built for it and a flag-1 job whose FIRST step out of int64 is that step, one
    grid unit of the cells apart; the V1 cut has both sides on both branches of k = min(r, room)."""
    wide = v is None
    u = 1 if wide else 1 << v
    reach = E.STEPS if wide or v >= 30 else ("mul", "acc")
    for mode, steps in ((V2, reach), (V1, ("v1 room", "v1 r"))):
        arrs, cases, sh = variant_batch(mode, v)
        first = E.model(mode, *arrs, 2)[4]
        vals, _, _, flag = checker(mode, arrs, 2)
        for step in steps:
            ins = [j for j, c in enumerate(cases) if c["step"] == step and c["side"] == "in"]
            outs = [j for j, c in enumerate(cases) if c["step"] == step and c["side"] == "out"]
            assert ins and outs, (step, v)
            assert all(flag[j] == 0 and first[j] is None for j in ins), step
            want_first = "mul" if step.startswith("v1") else step
            assert all(flag[j] == 1 and first[j] == want_first for j in outs), (step, [first[j] for j in outs])
            for i, o in zip(ins, outs):                     # the pair: the same job one grid unit on
                assert cases[i]["name"] == cases[o]["name"]
                assert 0 < abs(cases[o]["want"] - cases[i]["want"]) <= u * cases[i]["kabs"], cases[i]["name"]
                assert not -E.LIM <= cases[o]["want"] < E.LIM and -E.LIM <= cases[i]["want"] < E.LIM
        if mode == V2:
            got = {c["step"] for c in cases}
            assert {"max", "members", "presence"} <= got
            if wide or v <= 32:                             # -2^63 itself is an answer
                assert any(c["want"] == -E.LIM and c["flag"] == 0 for c in cases)
            if wide:
                assert any(c["want"] == E.LIM - 1 and c["flag"] == 0 for c in cases)


@pytest.mark.parametrize("n_keys", [1, 4, 5, 8, 9, 16])
def test_packing_is_what_the_variant_claims(n_keys):
    """narrowable() holds for the union of ALL cells of a narrowed batch, filler and oversized job included
    (so for every segment: a subset's OR spans no more than the whole), with the edge in every key on its
    own shift; and fails for every single job of the unnarrowable batch (the absent wide cell)."""
    for mode in (V1, V2):
        for rot in range(len(E.SHIFTS) if n_keys == 1 else 2):
            sh = E.key_shifts(n_keys, rot)
            arrs, cases = E.edge_batch(mode, n_keys, sh)
            cells = np.concatenate([arrs[4], E.filler_batch(300, n_keys, 5 + rot, sh)[4], E.oversized_job(n_keys, sh)[4]])
            assert E.narrowable(cells, n_keys)
            assert [E.ctz(x) for x in E.key_or(arrs[4], n_keys)] == sh     # every key's shift is its own
            assert {c["key"] for c in cases} == set(range(n_keys))
        arrs, cases = E.edge_batch(mode, n_keys, None)
        jgo, gco = arrs[0], arrs[3]
        for j in range(len(cases)):
            assert jgo[j + 1] > jgo[j]
            assert not E.narrowable(arrs[4][gco[jgo[j]]:gco[jgo[j + 1]]], n_keys), cases[j]["name"]
    for narrow in (True, False):
        for out in (False, True):
            arrs, total = E.oversized_edge(n_keys, n_keys - 1, narrow, out)
            assert E.narrowable(arrs[4], n_keys) == narrow
            assert total == (E.LIM if out else E.LIM - (1 << 31 if narrow else 1))
            assert E.seg_bytes(1, 1, 4096, True, E.nd_of(n_keys), 4, narrow) > E.SEG_BYTES
    assert E.saves_bytes(2, 4) and not E.saves_bytes(1, 4) and not E.saves_bytes(0, 16) and E.saves_bytes(1, 8)


@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("n_keys", [1, 4, 5, 8, 9, 16])
def test_key_table_batches(mode, n_keys):
    """The batches of the GPU tests (the edge in every key, key 0 and the last one among them): checker ==
    oracle == hand values, no flag 2."""
    for sh in (None, E.key_shifts(n_keys, 0), E.key_shifts(n_keys, 5)):
        arrs, cases = E.edge_batch(mode, n_keys, sh)
        vals, pres, mem, flag = checker(mode, arrs, n_keys)
        o = oracle.pg_min_resources_keys(mode, *arrs)
        assert not (flag == 2).any()
        np.testing.assert_array_equal(flag, o[3])
        np.testing.assert_array_equal(pres, o[1])
        np.testing.assert_array_equal(mem, o[2])
        np.testing.assert_array_equal(vals[flag == 0], o[0][flag == 0].astype(object))
        for j, c in enumerate(cases):
            assert (flag[j], vals[j, c["key"]], mem[j]) == (c["flag"], c["want"], c["mem"]), c["name"]


@pytest.mark.parametrize("fault", sorted(E.FAULTS))
def test_every_fault_is_caught(fault):
    """Each fault differs from the checker on at least one job of every variant and mode in which it can
    show (agg_edges.fault_applies says where it cannot, and why) -- and where it cannot, it does not."""
    applied = 0
    for mode in (V1, V2):
        for v in VARIANTS:
            arrs, cases, sh = variant_batch(mode, v)
            want = E.int64_answers(checker(mode, arrs, 2))
            same = E.same_answers(E.model(mode, *arrs, 2, fault=fault, pack=sh is not None), want)
            if E.fault_applies(fault, mode, sh and sh[:1], sh and sh[1:]):
                applied += 1
                assert not same.all(), (fault, mode, v)
            else:
                assert same.all(), (fault, mode, v, [cases[j]["name"] for j in np.flatnonzero(~same)])
    assert applied >= 2


@pytest.mark.parametrize("n_keys", [1, 4, 5, 8, 9, 16])
def test_kernel_argument_route_is_taken(n_keys):
    """Which one-job calls travel in the kernel arguments: a job's segment (narrowed when narrow_seg would
    narrow it) of at most 512 B.  At every width, in every variant and mode, each overflow step and each
    branch of the V1 cut has a job on EACH side of int64 that does; the jobs that do not (wide records with
    four containers and more) take the pinned segment with and without PE_AGG_NO_KARG."""
    nd = E.nd_of(n_keys)
    for mode in (V1, V2):
        for sh in (None, E.key_shifts(n_keys, 0), E.key_shifts(n_keys, 5)):
            arrs, cases = E.edge_batch(mode, n_keys, sh, sorted({0, n_keys - 1}))
            ng, nc = E.job_sizes(arrs)
            jgo, gco = arrs[0], arrs[3]
            fits = []
            for j in range(len(cases)):
                cells = arrs[4][gco[jgo[j]]:gco[jgo[j + 1]]]
                narrow = E.saves_bytes(nc[j], nd) and E.narrowable(cells, n_keys)
                assert narrow == (sh is not None and E.saves_bytes(nc[j], nd))
                fits.append(E.seg_bytes(1, ng[j], nc[j], mode == V1, nd, 4, narrow) <= 512)
            for key in {c["key"] for c in cases}:
                sides = {(c["step"], c["side"]) for c, f in zip(cases, fits) if f and c["key"] == key}
                need = {(c["step"], c["side"]) for c in cases if c["side"] != "one" and c["key"] == key}
                assert need and need <= sides, (mode, sh, key, sorted(need - sides))
            assert nd == 16 or sum(fits) > 0.9 * len(fits)
            if nd == 16 and sh is None:
                assert not all(fits)                        # (four 128-B records: the pinned segment)


@pytest.mark.parametrize("n_keys", [1, 4, 5, 8, 9, 16])
def test_small_filler_fills_a_256_job_segment(n_keys):
    """255 small filler jobs and an edge job stay below the byte limit at every key width, so the first
    edge job aiming at lane 255 gets it -- with random_keys_csr filler alone no table wider than 4 keys
    ever fills a segment.  Every small job has the containers from which a narrowed segment saves bytes."""
    for mode in (V1, V2):
        for sh in (None, E.key_shifts(n_keys, 3)):
            edge, cases = E.edge_batch(mode, n_keys, sh, sorted({0, n_keys - 1}), pad=2)
            small = E.small_filler(2 * E.SEG_JOBS, n_keys, 9, sh)
            assert E.saves_bytes(min(E.job_sizes(small)[1]), E.nd_of(n_keys))
            assert sh is None or E.narrowable(np.concatenate([edge[4], small[4]]), n_keys)
            filler = E.filler_batch(700, n_keys, 4, sh, min_cont=2)
            arrs, pos, reached, full = E.assemble(edge, filler, n_keys, E.SEG_JOBS, mode == V1, small=small)
            assert reached["last"] >= 1 and full
            pl = E.Planner(E.SEG_JOBS, mode == V1, E.nd_of(n_keys), 4)
            lanes = [pl.add(g, c) for g, c in zip(*E.job_sizes(arrs))]
            assert lanes[pos[1]] == E.SEG_JOBS - 1 and len(lanes) == len(cases) + 700 + 2 * E.SEG_JOBS
            _, _, r2, f2 = E.assemble(edge, filler, n_keys, E.SEG_JOBS, mode == V1)
            assert n_keys <= 4 or (r2["last"] == 0 and not f2)


def test_planner_restated():
    """assemble() places edge jobs where it says: lane 0, the last lane and directly after the oversized
    job, with 32-job segments.  This replays assemble's bookkeeping through Planner; that Planner is the
    engine's rule rests on reading agg_call_locked's `plan` and agg_seg_layout beside it, and on the GPU
    tests' segment counts -- for ONE job range: from 32768 jobs on the engine cuts the batch at chunk
    and thread edges first, which Planner does not model."""
    sh = E.key_shifts(4, 0)
    edge, cases = E.edge_batch(V2, 4, sh, edge_keys=[0])
    edge = E.csr_slice(edge, 0, 12)
    filler = E.filler_batch(2048 - 13, 4, 3, sh)
    arrs, pos, reached, full = E.assemble(edge, filler, 4, 32, False, big=E.oversized_job(4, sh))
    assert len(arrs[0]) - 1 == 2048 and len(pos) == 12 and full
    assert reached == {"first": 7, "last": 4, "after_big": 1}   # (one job follows the big one; the next aim at lane 0)
    for i, p in enumerate(pos):                             # the edge jobs arrive unchanged
        a, b = E.csr_slice(arrs, p, p + 1), E.csr_slice(edge, i, i + 1)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    pl = E.Planner(32, False, 4, 4)                         # replayed: the lanes are the planner's
    ng, nc = E.job_sizes(arrs)
    lanes = [pl.add(g, c) for g, c in zip(ng, nc)]
    assert sum(lanes[p] == 0 for p in pos) == 8 and sum(lanes[p] == 31 for p in pos) == 4
    assert lanes[pos[2]] == 0 and E.seg_bytes(1, ng[pos[2] - 1], nc[pos[2] - 1], False, 4, 4) > E.SEG_BYTES
