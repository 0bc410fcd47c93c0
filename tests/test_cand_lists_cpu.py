"""cand_lists.py on the CPU: the reference against brute force on tiny inputs, the preconditions of every generated
case, and that every case named for a selection regime of topk_sort reaches that regime under the bin arithmetic
restated in cand_lists.regime -- a later change of MG_SEL or of a generator cannot turn them into direct-sort cases
unnoticed."""
import itertools
import os
import struct

import pytest

import cand_lists as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = {name: make() for name, make in cl.SUITES.items()}


def test_constants_match_the_header():
    h = cl.header_constants(os.path.join(ROOT, "training-operator_amd", "csrc", "pe_kernels.h"))
    assert h == {"MG_CAP": cl.MG_CAP, "MG_THREADS": cl.MG_THREADS, "MG_SEL": cl.MG_SEL, "RM_MAX_WORLD": cl.RM_MAX_WORLD,
                 "RM_MAX_LDS": cl.RM_MAX_LDS, "CAND_TIMEOUT": cl.CAND_TIMEOUT, "CAND_CORRUPT": cl.CAND_CORRUPT}


def brute(S, bound, K):
    """Tight by search: of all sound (list, limit) with at most K keys, the longest list and then the largest limit.
    A sound answer lists every key of S below its limit, so it is a prefix of sorted S and its limit is at most the
    next key -- and at most the bound, beyond which the kernel knows nothing."""
    srt = sorted(S)
    best = None
    for m in range(min(K, len(srt)) + 1):
        if m and srt[m - 1] >= bound:
            break
        limit = min(bound, srt[m]) if m < len(srt) else bound
        assert all((k in srt[:m]) for k in S if k < limit)
        best = (m, limit, srt[:m])
    return best


def test_reference_is_the_brute_force_answer_on_tiny_inputs():
    vals = [cl.MIN_KEY + v for v in (1, 2, 4, 7, 8)]
    n = 0
    for r in range(len(vals) + 1):
        for S in itertools.combinations(vals, r):
            for bound in [cl.MIN_KEY + b for b in (0, 1, 3, 7, 8, 9)] + [cl.NO_KEY]:
                for K in (1, 2, 3, 5, 6):
                    assert cl.tight(list(S), bound, K) == brute(S, bound, K), (S, bound, K)
                    n += 1
    assert n > 1000


def test_reference_of_the_documented_exceptions():
    K = 4
    ok = (2, cl.NO_KEY, [cl.MIN_KEY + 1, cl.MIN_KEY + 9])
    for kind in cl.SHARD_KINDS:
        for bad_n in (-1, K + 1):
            c = cl.Case("x", kind, 2, K, [[ok, (bad_n, cl.NO_KEY, [cl.MIN_KEY + 2])]], gen=0x80000002)
            e = cl.reference(c, 0)
            assert (e.n, e.flags, e.limit, e.keys) == (cl.CAND_CORRUPT, -(1 << 31) + 2, 0, [])
        c = cl.Case("x", kind, 2, K, [[ok, ok]], gen=3, xstatus=cl.XSTATUS)
        e = cl.reference(c, 0)
        assert (e.n, e.flags, e.limit, e.keys) == (cl.CAND_TIMEOUT, 3, cl.XSTATUS, [])
    keys = list(range(cl.MIN_KEY + 5, cl.MIN_KEY + 5 + cl.MG_CAP + 1))
    waves = [(64, cl.NO_KEY, keys[i:i + 64]) for i in range(0, len(keys) - 1, 64)] + [(1, cl.NO_KEY, keys[-1:])]
    e = cl.reference(cl.Case("x", cl.MERGE, len(waves), K, [waves]), 0)
    assert (e.n, e.flags, e.limit, e.keys) == (1, 1, cl.MIN_KEY + 6, [cl.MIN_KEY + 5])
    e = cl.reference(cl.Case("x", cl.MERGE, len(waves) - 1, K, [waves[:-1]]), 0)      # MG_CAP keys exactly: a list
    assert (e.n, e.flags, e.limit, e.keys) == (K, 0, keys[K], keys[:K])
    e = cl.reference(cl.Case("x", cl.EMPTY, 1, K, [None], gen=5), 0)
    assert (e.n, e.flags, e.limit, e.keys) == (0, 5, cl.NO_KEY, [])


def test_regime_restates_topk_sort_on_hand_made_inputs():
    b = 1 << 40
    assert cl.regime([b + i for i in range(2 * 9 + 2)], 9)[0] == "direct"
    assert cl.regime([b + i for i in range(2 * 9 + 3)], 9)[0] == "one"
    assert cl.regime([b + i for i in range(1024)], 511)[0] == "direct"       # T <= 2 (K + 1) and T <= MG_SEL
    assert cl.regime([b + i for i in range(1025)], 600)[0] != "direct"       # T <= 2 (K + 1), T > MG_SEL
    assert cl.regime([b + i for i in range(3000)], 1024)[0] == "bitonic"     # K + 1 > MG_SEL
    name, p = cl.regime([b + 3 * i for i in range(86)], 7)                   # range 255: one key value per bin
    assert (name, p["bits"], p["sh"], p["cb"], p["before"], p["sel_c"]) == ("one", 8, 0, 21, 7, 8)
    name, p = cl.regime([b + 3 * i for i in range(87)], 7)                   # range 258: bins of two values
    assert (name, p["bits"], p["sh"], p["cb"], p["before"], p["sel_c"]) == ("one", 9, 1, 10, 7, 8)
    # 2000 keys in the first 2^16 of a 2^32 range, 16 apart: bin 0 (2^24 wide) holds them all, sub-bins of 2^16 too
    keys = [b + 16 * i for i in range(2000)] + [b + (1 << 32) - 1]
    name, p = cl.regime(keys, 300)
    assert (name, p["sh"], p["cb"], p["sel_c"], p["sh2"], p["cb2"], p["C"]) == ("bitonic", 24, 0, 2000, 16, 0, 2000)
    keys = [b + 4096 * i for i in range(2000)] + [b + (1 << 32) - 1]         # 16 per sub-bin: the cut is sub-bin 18
    name, p = cl.regime(keys, 300)
    assert (name, p["cb2"], p["C"]) == ("two", 18, 19 * 16)


@pytest.mark.parametrize("suite", sorted(ALL))
def test_every_case_keeps_what_the_kernels_assume(suite):
    cases = ALL[suite]
    assert cases
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids)
    for c in cases:
        cl.check_preconditions(c)
        overflow = c.kind == cl.MERGE and any(cl.reference(c, g).flags == 1 for g in range(c.Wg))
        assert overflow == (c.name in ("at_cap", "overflow_300_full")), c.id


def test_named_cases_reach_their_regime():
    seen = {}
    for c in ALL["regimes"] + ALL["grid"]:
        for g, (want, props) in c.regimes.items():
            got, p = cl.regime(cl.selected_keys(c, g), c.K)
            if want == "not_direct":
                assert got != "direct", (c.id, g, got)
            else:
                assert got == want, (c.id, g, got, p)
            for key, val in props.items():
                if key != "T":
                    assert p[key] == val, (c.id, g, key, p)
            seen.setdefault(c.name, set()).add(got)
    names = {name: reg for name, _, _, (reg, _) in cl.regime_keysets()}
    assert len(names) == 14 and all(seen[n] == {r} for n, r in names.items()), seen
    for kind in (cl.MERGE_SHARDS, cl.MERGE):      # every regime through both kernels
        got = {cl.regime(cl.selected_keys(c, 0), c.K)[0] for c in ALL["regimes"] if c.kind == kind}
        assert got == {"one", "two", "bitonic"}, got
    # the grid: every K at every edge T that some rank count admits, the direct sort up to 2K + 2 and MG_SEL
    for K in cl.GRID_K:
        Ts = {p["T"]: want for c in ALL["grid"] if c.K == K for want, p in c.regimes.values()}
        assert sorted(Ts) == sorted(set(cl.grid_T(K))), (K, Ts)
        assert all((want == "direct") == (T <= 2 * K + 2 and T <= cl.MG_SEL) for T, want in Ts.items())


def test_the_cases_cover_what_they_are_named_for():
    lim = dict(cl.limit_groups())
    case = [c for c in ALL["limits"] if c.name == "limits_w3"][0]
    ref = {what: cl.reference(case, g) for g, what in enumerate(lim)}
    K = case.K
    L = ref["exactly K keys below L"].limit
    assert L != cl.NO_KEY and ref["exactly K keys below L"].n == K
    assert ref["exactly K + 1 keys below L"].n == K and ref["exactly K + 1 keys below L"].limit < L
    assert ref["L is NO_KEY, fewer than K keys"].n < K and ref["L is NO_KEY, fewer than K keys"].limit == cl.NO_KEY
    assert ref["L is NO_KEY, more than K keys"].n == K and ref["L is NO_KEY, more than K keys"].limit != cl.NO_KEY
    cut = lim["L cuts listed keys of the other ranks"]
    assert sum(1 for n, _, keys in cut[1:] for k in keys if k >= L) >= 2
    assert ref["a weak list: K - 1 keys and a real limit"].n == K - 1
    assert ref["every rank empty"].n == 0 and ref["every rank empty"].limit == cl.NO_KEY
    assert ref["an empty rank with a real limit"].n == 3
    assert ref["one rank holds everything"].n == K
    # merge_ranked: the U cut applies to the balanced lists and not beside empty ones; the search counts are reached
    for c in ALL["ranked"]:
        if c.name.startswith("shapes_w") and c.world > 1:
            c_head = -(-(c.K + 1) // c.world)
            heads = [sum(min(n, c_head) for n, _, _ in lists) for lists in c.groups]
            assert heads[0] >= c.K + 1 and heads[1] < c.K + 1, c.id
        if c.name == "search_counts":
            c_head = -(-(c.K + 1) // c.world)
            assert all(sum(min(n, c_head) for n, _, _ in lists) < c.K + 1 for lists in c.groups)
            assert {n for lists in c.groups for n, _, _ in lists} >= set(cl.SEARCH_COUNTS)
    assert {c.world for c in ALL["ranked"]} >= {1, 2, 3, 5, 8, 16}
    assert cl.merge_ranked_lds(16, 481) <= cl.RM_MAX_LDS < cl.merge_ranked_lds(16, 482)
    # merge: the wave counts run from 0 to 64, some bound cuts keys of other waves, keys are not in order
    assert {c.world for c in ALL["merge"]} >= {1, 16, 1024, 1025, 2000}
    counts, cuts, unordered = set(), 0, 0
    for c in ALL["merge"]:
        for waves in c.groups:
            S, G = cl.wave_keys(waves)
            counts |= {n for n, _, _ in waves}
            cuts += any(k >= G for k in S)
            unordered += any(keys != sorted(keys) for _, _, keys in waves)
    assert counts == set(range(65)) and cuts >= 10 and unordered >= 10


def test_blob_writer_and_reader_round_trip(tmp_path):
    """The case file's layout, and check_output on an output made from the reference: exact passes, and a wrong key,
    a low limit, a short list, a stray store past n or into the guard are each reported."""
    cases = [c for c in ALL["every_kind"] if c.name in ("stride_gen", "corrupt_minus1", "xstatus")][:3] + ALL["refused"][:1]
    cases += [c for c in ALL["merge"] if c.name == "overflow_300_full"]
    path = str(tmp_path / "cases.bin")
    cl.write_cases(path, cases)
    raw = open(path, "rb").read()
    assert struct.unpack_from("<II", raw, 0) == (cl.MAGIC, len(cases))
    c0 = cases[0]
    hdr = struct.unpack_from("<7qQ4q", raw, 8)
    assert hdr[:7] == (c0.kind, c0.world, c0.Wg, c0.K, c0.rank_stride, c0.gen, 0) and hdr[9] == c0.Wg * cl.group_bytes(c0.K)
    data = raw[8 + 96:8 + 96 + hdr[8]]
    n, _, lim = struct.unpack_from("<iiQ", data, c0.rank_stride + cl.group_bytes(c0.K))      # rank 1, group 1
    assert (n, lim) == c0.groups[1][1][:2]
    assert data[c0.Wg * cl.group_bytes(c0.K):c0.rank_stride] == bytes([cl.FILLER]) * 136

    def perfect(c):
        buf = bytearray([cl.FILL]) * (c.Wg * cl.group_bytes(c.K) + cl.GUARD)
        if not c.refused:
            for g in range(c.Wg):
                e = cl.reference(c, g)
                struct.pack_into("<iiQ%dQ" % len(e.keys), buf, g * cl.group_bytes(c.K), e.n, e.flags, e.limit, *e.keys)
        return (cl.HIP_INVALID_VALUE if c.refused else 0, 0, bytes(buf))

    out = str(tmp_path / "out.bin")
    with open(out, "wb") as f:
        f.write(struct.pack("<II", cl.MAGIC, len(cases)))
        for c in cases:
            le, se, buf = perfect(c)
            f.write(struct.pack("<iiq", le, se, len(buf)) + buf)
    results = cl.read_outputs(out, cases)
    for c, r in zip(cases, results):
        assert cl.check_output(c, r) == [], c.id
    gb = cl.group_bytes(c0.K)
    good = bytearray(results[0][2])
    e = cl.reference(c0, 0)
    assert e.n >= 2

    def judged(edit):
        buf = bytearray(good)
        edit(buf)
        return cl.check_output(c0, (0, 0, bytes(buf)))

    assert judged(lambda b: struct.pack_into("<Q", b, 16, e.keys[0] + 1))                   # a wrong key
    assert judged(lambda b: struct.pack_into("<Q", b, 8, e.limit - 1))                      # a low limit (sound, not tight)
    assert judged(lambda b: struct.pack_into("<i", b, 0, e.n - 1))                          # a short list
    assert judged(lambda b: struct.pack_into("<i", b, 4, 0))                                # flags
    assert judged(lambda b: struct.pack_into("<B", b, gb - 1, 0))                           # a store past n
    assert judged(lambda b: struct.pack_into("<B", b, len(b) - 1, 0))                       # the guard
    assert cl.check_output(cases[3], (0, 0, results[3][2])) and cl.check_output(c0, (0, 700, results[0][2]))
