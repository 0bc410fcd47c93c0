"""pe_place_skew_domains on the device against the rule pod by pod in Python integers: every pod slot, status and
residual cell, exact.  The reference also says which situations of the device's decision a batch reaches (`seen`);
the tests assert them on the reference: a condition on the inputs, not on the device."""
import numpy as np
import pytest

import domain_placement as DP
import tree_capacity as TC
from oracle import semantics as S
from placement import PE_SKEW_NONE, PE_SPREAD_NODE, Engine, _abi, synth

pytestmark = pytest.mark.gpu

GiB, ISLAND, NODE, NONE = DP.GiB, DP.ISLAND, PE_SPREAD_NODE, PE_SKEW_NONE
SK_LDS_NODES = 845                          # pe_kernels.h
GPU1, QS, Q, ZERO, GOLD = [1000, GiB, 1, 0], [500, GiB, 0, 0], [16000, 64 * GiB, 0, 0], [0, 0, 0, 0], 2


def skew_python(case, skews, base, spread_level):
    """(pods, status, residual [4][N], seen) by the rule of include/placement.h, one pod at a time: place_python's
    loop with the cnt / gmin predicate in the fit.  base: (group_base_off, base_dom, base_count) or None."""
    b, labels = case.batch, [int(x) for x in case.labels]
    R = [[int(x) for x in row] for row in case.residual()]
    dom = DP.dom_level(case.island, case.level, case.level_size, case.parent)
    sd = list(range(len(dom))) if spread_level < 0 else [int(x) for x in DP.dom_level(case.island, spread_level, case.level_size, case.parent)]
    poff = DP.pod_offsets(b.group_count)
    pods, status, seen = [-1] * poff[-1], [0] * len(b.priority), set()
    for j in sorted(range(len(status)), key=lambda j: (-int(b.priority[j]), j)):
        placed, cands = [], [n for n, d in enumerate(dom) if d == case.job_domain[j]]
        for g in range(int(b.job_group_off[j]), int(b.job_group_off[j + 1])):
            q, need, c = [int(x) for x in b.group_req[g]], int(b.group_need[g]), int(b.group_count[g])
            s = None if skews is None or skews[g] == NONE else int(skews[g])
            unit = max(c, 1) if need & ISLAND else 1    # an island group: one step of `unit` pods
            qe = [x * unit for x in q]
            cnt = {sd[n]: 0 for n in cands if labels[n] & need == need}          # the eligible spread domains
            for e in range(*(base[0][g:g + 2] if base else (0, 0))):
                if int(base[1][e]) in cnt:
                    cnt[int(base[1][e])] += int(base[2][e])
            if s is not None and c and len({sd[n] for n in cands}) > len(cnt) > 0 and min(cnt.values()) > 0:
                seen.add("ineligible domain does not hold the minimum down")
            run = None                                  # (node, pods, began as the only minimum, m2 then)
            for p in range(0, c, unit):
                fit = {n: S.appendix_b_key([R[d][n] for d in range(4)], labels[n], qe, need, n) for n in cands} \
                    if max(qe) <= S.INT64_MAX else {}
                fit = {n: k for n, k in fit.items() if k is not None}
                low = sorted(cnt.values())[:2] + [None, None]
                if s is None:
                    ok = fit
                elif unit > 1 or need & ISLAND:         # the minimum over the other eligible spread domains
                    other = lambda u: low[1] if cnt[u] == low[0] else low[0]   # noqa: E731
                    ok = {n: k for n, k in fit.items() if other(sd[n]) is None or cnt[sd[n]] + unit - other(sd[n]) <= s}
                    seen.add("island unit within its bound" if ok else "island unit beyond its bound" if fit else "")
                else:
                    ok = {n: k for n, k in fit.items() if cnt[sd[n]] + 1 - low[0] <= s}
                n = min(ok, key=ok.get) if ok else None
                if s is not None and not need & ISLAND:   # what the device's take-many has to get right
                    if run and run[0] != n and run[1] >= 2 and not run[2]:
                        seen.add("run cut by take_of" if run[0] not in fit else "run cut by A" if run[0] not in ok else "")
                    if run and run[0] != n and n is not None and run[0] in ok:
                        seen.add("a newly admitted node wins")
                    if n is None and fit and not any(cnt[sd[m]] == low[0] for m in fit):
                        seen.add("full eligible domain fails the gang")
                    if n is not None:
                        only = cnt[sd[n]] == low[0] and low[1] != low[0]
                        if only and ok[n] != min(fit.values()):
                            seen.add("only minimum, not the unconstrained argmin")
                        if run and run[0] == n and run[2] and run[3] is not None and cnt[sd[n]] >= run[3]:
                            seen.add("run across m2")
                        run = (n, run[1] + 1, run[2], run[3]) if run and run[0] == n else \
                            (n, 1, only and ok[n] == min(fit.values()), low[1])
                if n is None:
                    break
                cnt[sd[n]] += unit
                for d in range(4):
                    R[d][n] -= qe[d]
                pods[poff[g] + p:poff[g] + p + unit] = [n] * unit
                placed.append((g, n, unit))
            else:
                if s is not None and run and run[1] >= 2 and not run[2]:
                    seen.add("run cut by left")
                continue
            if len({sd[n] for _, n, _ in placed}) >= 2:
                seen.add("rollback over several domains")
            for g2, n, u in placed:                     # all or nothing
                for d in range(4):
                    R[d][n] += u * int(b.group_req[g2][d])
            lo, hi = poff[int(b.job_group_off[j])], poff[int(b.job_group_off[j + 1])]
            pods[lo:hi], status[j] = [-1] * (hi - lo), 1
            break
    return np.array(pods, dtype=np.int32), np.array(status, dtype=np.int32), np.array(R, dtype=np.int64), seen - {""}


def make_case(size, kind, jobs=()):
    """(case, spread_level, sd_of): domain 0 of `size` nodes and domain 1 of 5 in a shuffled order, 3 nodes in none.  "node":
    one level, hostname spread.  "rack": blocks (level 1) over racks of a half, a quarter, an eighth and the rest of a
    block's nodes, spread per rack.  Node k of a domain has 8 free GPUs, 7 where k % 8 == 6, 6 for k == 2 (its domain's
    best fit) and 0 -- full -- where k % 8 == 4 and, for "rack", in the whole last rack.  Every fourth node carries GOLD,
    for "rack" only in the first rack.  sd_of(k): the spread domain of node k of domain 0."""
    rack_in = lambda k, s: min(3, int(np.log2(s / max(s - k, 1))))   # noqa: E731  (0: the first half, 1: the next quarter ...)
    ks = np.array(list(range(size)) + list(range(5)) + [0] * 3)
    racks = np.array([rack_in(k, size) for k in range(size)] + [4 + rack_in(k, 5) for k in range(5)] + [-1] * 3, np.int32)
    order = np.random.default_rng(size).permutation(len(racks))
    ks, racks = ks[order], racks[order]
    full = (ks % 8 == 4) | ((kind == "rack") & (racks % 4 == 3))
    gpus = np.where(full, 0, np.where(ks == 2, 6, np.where(ks % 8 == 6, 7, 8)))
    free = np.array([[64000] * len(ks), [256 * GiB] * len(ks), gpus, [0] * len(ks)], dtype=np.int64)
    labels = synth.island_labels(np.where((ks % 4 == 0) & ((kind == "node") | (racks % 4 == 0)), 1 | GOLD, 1), racks)
    batch, job_domain = DP.make_batch(jobs)
    if kind == "node":
        node_of = {int(k): n for n, (k, r) in enumerate(zip(ks, racks)) if 0 <= r < 4}
        island = np.where(racks < 0, -1, racks // 4).astype(np.int32)
        return DP.Case(free, np.zeros_like(free), labels, island, [2], None, 0, batch, job_domain), NODE, node_of.get
    parent = np.array([0] * 4 + [1] * 4, np.int32)
    return DP.Case(free, np.zeros_like(free), labels, racks, [8, 2], parent, 1, batch, job_domain), 0, lambda k: rack_in(k, size)


# the only minimum holds the best fit and runs across m2 (g0); it does not: single pods until a node let in wins (g1); pods on
# several spread domains, then no fit, and a lower-priority job on what came back (g2 - g4); island units of 1 and 3 pods (g5, g6); a zero
# request (g7); a label only some spread domains carry, over a book that covers them (g8) or leaves the full ones at 0 (g9); runs (g10); the small domain (g11)
NO_FIT = (1, [1, 0, 0, 0], DP.NO_LABEL)
JOBS = [(0, 20, [(5, GPU1, 0)]), (0, 19, [(4, GPU1, 0)]), (0, 9, [(3, GPU1, 0), NO_FIT]), (0, 8, [(6, GPU1, 0)]),
        (0, 7, [(1, QS, ISLAND), (3, QS, ISLAND)]), (0, 6, [(20, ZERO, 0)]), (0, 5, [(7, GPU1, GOLD)]), (0, 5, [(2, GPU1, GOLD)]),
        (0, 4, [(8, GPU1, 0)]), (1, 3, [(3, GPU1, 0)])]
SKEWS = {"1": [1] * 12, "2": [2] * 12, "none": [NONE] * 12, "mixed": [1, 2, NONE, 1, 2, 1, 3, 1, 1, 1, 4, NONE]}
SIZES = [1, 2, 255, 257, SK_LDS_NODES - 1, SK_LDS_NODES, SK_LDS_NODES + 1]   # + 1: the in-place instance
SEEN = {"run across m2", "only minimum, not the unconstrained argmin", "a newly admitted node wins", "island unit within its bound",
        "ineligible domain does not hold the minimum down", "rollback over several domains"}
SEEN = {"1": SEEN | {"island unit beyond its bound", "full eligible domain fails the gang"}, "none": set(),
        "2": SEEN | {"island unit beyond its bound", "run cut by A", "run cut by left"}, "mixed": SEEN | {"run cut by A", "run cut by left", "run cut by take_of"}}


def make_book(case, size, sd_of):
    """The books of g0, g1, g8 and g9 over domain 0's spread domains, with duplicates (1 + 2) and, in g0, an entry
    outside the job's domain: a spread domain of domain 1 with no pods, which would hold the minimum at 0."""
    sds = sorted({sd_of(k) for k in range(size)})
    gold, ku = [k for k in range(size) if k % 4 == 0], (size // 2 + 8) // 8 * 8 + 1   # ku: not full, in the second rack
    book = {0: [(u, c) for u in sds if u != sd_of(2) for c in (1, 2)] + [(sd_of(2), 1)] * (size > 2),
            1: [(u, 2) for u in sds if u != sd_of(ku)] * (size > ku),
            8: [(sd_of(k), 1) for k in gold] if case.level == 0 else [(0, 2)],
            9: [(sd_of(k), 1) for k in gold if k % 8 == 0] if case.level == 0 else [(0, 1)]}
    outside = int(np.nonzero(case.island == 1)[0][0]) if case.level == 0 else 5
    book[0] = book[0] + [(outside, 0)]
    flat = [e for g in range(12) for e in book.get(g, [])]
    return [sum(len(book.get(h, [])) for h in range(g)) for g in range(13)], [u for u, _ in flat], [c for _, c in flat]


def call(eng, case, skews, base, spread_level, dry_run=False):
    b = case.batch
    return eng.place_skew_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, skews, spread_level,
                                  case.job_domain, case.level, case.level_size, case.parent, base, dry_run)


def check(eng, case, skews, base, spread_level):
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    want = skew_python(case, skews, base, spread_level)
    pods, st = call(eng, case, skews, base, spread_level)
    assert st.tolist() == want[1].tolist() and np.array_equal(pods, want[0]) and np.array_equal(eng.read_residuals(), want[2])
    return want


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("skews", list(SKEWS))
@pytest.mark.parametrize("kind", ["node", "rack"])
@pytest.mark.parametrize("size", SIZES)
def test_against_the_rule(eng, size, kind, skews):
    case, spread_level, sd_of = make_case(size, kind, JOBS)
    want = check(eng, case, np.array(SKEWS[skews], np.int32), make_book(case, size, sd_of), spread_level)
    assert size < 255 or (want[3] >= SEEN[skews] and want[1][2] == 1 and want[1][3] == (kind == "rack" and skews == "1")), want[3]


@pytest.mark.parametrize("skew,book,gpus,pods", [   # the header's examples
    (1, None, [8, 8], [0, 1, 0, 1]), (2, None, [8, 8], [0, 0, 1, 0]), (1, ([0, 1], [1], [2]), [8, 8], [0, 0, 0, 1]),
    (1, None, [8, 0], None)])
def test_header_examples(eng, skew, book, gpus, pods):
    free = np.array([[64000] * 2, [256 << 30] * 2, gpus, [0] * 2], dtype=np.int64)
    case = DP.Case(free, free * 0, np.ones(2, np.uint32), np.zeros(2, np.int32), [1], None, 0, *DP.make_batch([(0, 0, [(4, GPU1, 0)])]))
    want = check(eng, case, [skew], book, NODE)
    assert (want[0].tolist(), want[1].tolist()) == ((pods, [0]) if pods else ([-1] * 4, [1]))
    b = case.batch                                          # a cap of 4 per node places what maxSkew 1 refuses
    assert pods or eng.place_spread_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, [4], NODE,
                                            case.job_domain, 0, [1], None, dry_run=True)[0].tolist() == [0] * 4


def test_identity_with_place_greedy_domains(eng):
    other = Engine(0)
    for level, spread_level, skews in ((0, NODE, None), (1, 0, True), (2, NODE, True), (2, 1, None)):
        case = DP.tree_case("racks32", 1025, level)
        eng.load_nodes(case.cap, case.used, case.labels, case.island)
        other.load_nodes(case.cap, case.used, case.labels, case.island)
        b = case.batch
        want = other.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need,
                                          case.job_domain, level, case.level_size, case.parent)
        got = call(eng, case, skews and np.full(len(b.group_count), NONE, dtype=np.int32), None, spread_level)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[1] == 0).any()
        assert np.array_equal(eng.read_residuals(), other.read_residuals())
    other.close()


@pytest.mark.parametrize("kind,size", [("node", 257), ("rack", SK_LDS_NODES + 1)])
def test_dry_run_then_commit_then_release(eng, kind, size):
    case, spread_level, sd_of = make_case(size, kind, JOBS)
    skews, book = np.array(SKEWS["mixed"], np.int32), make_book(case, size, sd_of)
    eng.load_nodes(case.cap, case.used, case.labels, case.island)
    before, stats, held = eng.read_residuals(), eng.stats(), [x.copy() for x in eng.gang_capacity([Q, QS])]
    dry = call(eng, case, skews, book, spread_level, dry_run=True)
    assert np.array_equal(eng.read_residuals(), before) and eng.stats() == stats
    assert all(np.array_equal(x, y) for x, y in zip(eng.gang_capacity([Q, QS]), held))
    got = call(eng, case, skews, book, spread_level)
    assert np.array_equal(got[0], dry[0]) and np.array_equal(got[1], dry[1]) and (got[1] == 0).any() and (got[1] == 1).any()
    b = case.batch                                         # the ledger hand-over: the outputs as they are
    assert eng.release_gangs(b.job_group_off, b.group_count, b.group_req, got[0]) == int((got[0] >= 0).sum())
    assert np.array_equal(eng.read_residuals(), before)


def test_refusals():
    island, sizes, parent = TC.tree("racks32", 300)        # [10, 3, 1]
    inv = synth.make_inventory(300, 71)
    pods, st = np.full(6, -77, dtype=np.int32), np.full(2, -77, dtype=np.int32)   # sentinels
    good = dict(off=[0, 1, 3], pri=[0, 1], cnt=[2, 1, 3], req=[Q, QS, Q], skew=[1, -1, 2], sl=0, boff=[0, 1, 1, 3], bdom=[9, 0, 0],
                bcnt=[1, 0, 2], flags=0, dom=[1, 2], level=1, n_levels=3, sizes=sizes, parent=parent, n_jobs=2)

    def answers(e, code, text, **change):
        a = dict(good, **change)
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int64 if k == "req" else np.int32)
               for k in ("off", "pri", "cnt", "req", "skew", "boff", "bdom", "bcnt", "dom", "sizes", "parent")}
        ptr = lambda k: None if arr[k] is None else arr[k].ctypes.data   # noqa: E731
        rc = e.lib.pe_place_skew_domains(e.h, a["n_jobs"], ptr("off"), ptr("pri"), ptr("cnt"), ptr("req"), None, ptr("skew"),
                                         a["sl"], ptr("boff"), ptr("bdom"), ptr("bcnt"), a["flags"], ptr("dom"), a["level"],
                                         a["n_levels"], ptr("sizes"), ptr("parent"), pods.ctypes.data, st.ctypes.data)
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg, change)
        assert ((pods == -77).all() and (st == -77).all()) == (code != _abi.PE_OK)   # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    e.load_nodes(inv.cap, inv.used, inv.labels, island)
    before, E = e.read_residuals(), _abi.PE_EINVAL
    for text, change in [("group_count: negative value at index 1", dict(cnt=[2, -1, 3])), ("n_jobs < 0", dict(n_jobs=-1)),
                         ("job_domain: value outside [0, level_size[level]) at index 1", dict(dom=[1, 3])),
                         ("level outside", dict(level=3)), ("parent is NULL", dict(parent=None)),
                         ("spread_level outside", dict(sl=-2)), ("spread_level outside", dict(sl=1)),
                         ("spread_level outside", dict(sl=0, level=0)),
                         ("group_max_skew: value 0 or below -1 at index 2", dict(skew=[1, -1, 0])),
                         ("group_max_skew: value 0 or below -1 at index 0", dict(skew=[-2, 0, 1], boff=[0, 2, 1, 3])),
                         ("group_base_off: negative or descending at index 2", dict(boff=[0, 2, 1, 3], bdom=[10, 0, 0])),
                         ("group_base_off: negative or descending at index 0", dict(boff=[-1, 1, 1, 3])),
                         ("base_dom or base_count is NULL", dict(bcnt=None)),
                         ("base_dom: value outside its level at index 1", dict(bdom=[9, 10, 0], bcnt=[1, -1, 2])),
                         ("base_dom: value outside its level at index 2", dict(sl=-1, bdom=[299, 0, 300])),
                         ("base_dom: value outside its level at index 0", dict(bdom=[-1, 0, 0])),
                         ("base_count: negative value at index 2", dict(bcnt=[1, 0, -1], flags=2)),
                         ("flags: unknown bits", dict(flags=2)), ("flags: unknown bits", dict(flags=0x80000001))]:
        answers(e, E, text, **change)
    assert np.array_equal(e.read_residuals(), before)
    s = Engine(0, rank=1, world_size=2, exchange=lambda b: b * 2)   # a 2-shard context
    s.load_nodes(inv.cap, inv.used, inv.labels, island)
    answers(s, E, "shard")
    s.close()
    answers(e, _abi.PE_OK, "")                             # the same arguments unchanged are accepted
    e.close()
