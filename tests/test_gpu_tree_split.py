"""pe_gang_split_tree on the GPU against the Python-integer checker (tests/tree_split.py): every cell of every
output of every job compared, nothing sampled, and the residuals before and after."""
import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
import tree_capacity as TC
import tree_split as TS
from placement import Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

FIELDS = TS.FIELDS


def engine_for(case):
    e = Engine(0)
    e.load_nodes(case.cap, case.used, case.labels, case.island)
    return e


def check(e, case, max_parts=None, max_level="case"):
    """One call against the checker, the residuals untouched; returns the engine's answer."""
    mp = case.max_parts if max_parts is None else max_parts
    ml = case.max_level if isinstance(max_level, str) else max_level
    before = e.read_residuals()
    got = e.gang_split_tree(case.req, case.need, case.count, ml, case.sizes, case.parent, mp)
    np.testing.assert_array_equal(e.read_residuals(), before)
    TS.same(got, TS.split(case.table, case.count, case.sizes, case.parent, ml, mp), f"max_parts {mp}")
    return got


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n_nodes", [1, 255, 257, 1025])
def test_sizes_and_trees(n_nodes, name):
    case = TS.named_case(name, n_nodes, strict=n_nodes > 1)
    e = engine_for(case)
    got = check(e, case)
    check(e, case, TS.MAX_PARTS)
    check(e, case, 1)
    # max_level NULL, and required at the leaf level / at level 1 for every job
    check(e, case, max_level=None)
    for r in (0, min(1, len(case.sizes) - 1)):
        check(e, case, TS.MAX_PARTS, np.full(len(case.count), r, dtype=np.int32))
    # the selection is pe_gang_capacity_tree's
    cap = e.gang_capacity_tree(case.req, case.need, case.count, case.max_level, case.sizes, case.parent, tables=False)
    np.testing.assert_array_equal(got.level, cap.level)
    np.testing.assert_array_equal(got.domain, cap.domain)
    if n_nodes >= 255 and len(case.sizes) > 1:
        assert (got.parts > 1).any() and (got.parts == TS.TOO_MANY).any() and (got.parts == 0).any()
    e.close()


@pytest.mark.parametrize("kind", TS.FAN_KINDS)
@pytest.mark.parametrize("fan_in", [1, 2, 3, 31, 32, 33, 63, 64, 65, 200])
def test_fan_in_boundaries(fan_in, kind):
    """One value per lane up to 64 children, strided passes beyond; ties, zeros and distinct slots."""
    case = TS.fan_case(fan_in, kind)
    e = engine_for(case)
    check(e, case)
    check(e, case, TS.MAX_PARTS)
    e.close()


@pytest.mark.parametrize("trap", TS.TRAPS, ids=[t[0] for t in TS.TRAPS])
def test_traps(trap):
    name, leaf, sizes, parent, count, parts, spread = trap
    case = TS.trap_case(trap)
    e = engine_for(case)
    got = check(e, case)
    n = len(parts)
    assert got.parts[0] == n and got.spread[0].tolist() == spread
    assert list(zip(got.part_domain[0, :n].tolist(), got.part_pods[0, :n].tolist())) == parts
    e.close()


def test_widest_level():
    """[65536, 1] with one node per leaf: the root's 65536 children in strided passes, up to 1024 parts."""
    rng = np.random.default_rng(8)
    leaf = rng.integers(0, 6, 65536)
    leaf[[5, 40000]] = 9
    cap, used, labels, island = TS.leaf_inventory(leaf)
    sizes, parent = [65536, 1], np.zeros(65536, dtype=np.int32)
    tab = np.concatenate([leaf, [leaf.sum()]]).astype(np.int64)[None]
    np.testing.assert_array_equal(TC.tables(cap[:, :300] - used[:, :300], labels[:300] | np.uint32(1 << 31), island[:300],
                                            [TS.GPU_REQ], None, [300, 1], np.zeros(300, dtype=np.int32))[0][0, :300], leaf[:300])
    fives = int((leaf == 5).sum())
    count = [1, 9, 10, 18, 19, 23, 18 + 5 * 1022, 18 + 5 * 1022 + 1, 18 + 5 * fives + 3, int(leaf.sum()), int(leaf.sum()) + 1]
    J = len(count)
    case = TS.Case(cap, used, labels, island, sizes, parent, np.tile(TS.GPU_REQ, (J, 1)), None, count, None, TS.MAX_PARTS,
                   np.repeat(tab, J, axis=0))
    e = engine_for(case)
    before = e.read_residuals()
    for mp in (TS.MAX_PARTS, 64):
        got = e.gang_split_tree(case.req, None, case.count, None, sizes, parent, mp)
        TS.same(got, TS.split_wide(tab, np.zeros(J, dtype=int), case.count, sizes, parent, None, mp), f"max_parts {mp}")
    assert got.parts.tolist()[:6] == [1, 1, 2, 2, 3, 3]
    full = e.gang_split_tree(case.req, None, case.count, None, sizes, parent, TS.MAX_PARTS)
    assert full.parts.tolist()[6:] == [1024, TS.TOO_MANY, TS.TOO_MANY, TS.TOO_MANY, 0]
    np.testing.assert_array_equal(e.read_residuals(), before)
    e.close()


def test_max_parts_boundary():
    """65 one-slot leaves, count 65: exactly 65 parts."""
    cap, used, labels, island = TS.leaf_inventory([1] * 65)
    sizes, parent = [65, 1], np.zeros(65, dtype=np.int32)
    tab = TC.tables(cap - used, labels | np.uint32(1 << 31), island, [TS.GPU_REQ], None, sizes, parent)[0]
    count = [65, 64, 2, 1, 66]
    case = TS.Case(cap, used, labels, island, sizes, parent, np.tile(TS.GPU_REQ, (5, 1)), None, count, None, 65,
                   np.repeat(tab, 5, axis=0))
    e = engine_for(case)
    for mp, parts in ((1, [-1, -1, -1, 1, 0]), (64, [-1, 64, 2, 1, 0]), (65, [65, 64, 2, 1, 0]), (1024, [65, 64, 2, 1, 0])):
        got = check(e, case, mp)
        assert got.parts.tolist() == parts
        assert got.part_domain.shape == (5, mp)
    assert got.part_domain[0, :65].tolist() == list(range(65)) and (got.part_pods[0, :65] == 1).all()
    assert (got.part_domain[0, 65:] == -1).all() and not got.part_pods[0, 65:].any()
    e.close()


def test_zero_request_and_largest_count():
    """A shape that asks for nothing holds PE_CAP_MAX pods per node; a gang of 2^31 - 1 fits one node's leaf."""
    n = 40
    inv = synth.make_inventory(n, 7)
    island = (np.arange(n) // 3).astype(np.int32)     # leaves of three nodes, the last of one
    sizes, parent = [14, 4, 1], np.array([k // 4 for k in range(14)] + [0] * 4, dtype=np.int32)
    req = np.zeros((3, 4), dtype=np.int64)
    count = np.array([2**31 - 1, 2**31 - 1, 1], dtype=np.int32)
    need = np.array([0, 1, 0], dtype=np.uint32)
    tab = TC.tables(inv.residual(), synth.island_labels(inv.labels, island), island, req, need, sizes, parent)[0]
    assert tab[0, 13] == 2**31 - 1 and tab[0, 0] == 3 * (2**31 - 1)
    case = TS.Case(inv.cap, inv.used, inv.labels, island, sizes, parent, req, need, count, None, 4, tab)
    e = engine_for(case)
    got = check(e, case)
    assert got.level[0] == 0 and got.domain[0] == 13 and got.part_pods[0, 0] == 2**31 - 1 and got.parts[0] == 1
    e.close()


def test_equal_shapes_under_different_counts():
    """The picks are the distinct (shape, count, max_level): shapes that recur out of order with other counts and
    levels, and exact repeats."""
    case = TS.named_case("four", 1025)
    rng = np.random.default_rng(5)
    J = len(case.count)
    order = rng.permutation(np.concatenate([np.arange(J), np.arange(J)[::3]]))
    ml = rng.integers(0, len(case.sizes), len(order)).astype(np.int32)
    mixed = TS.Case(case.cap, case.used, case.labels, case.island, case.sizes, case.parent, case.req[order],
                    case.need[order], case.count[order], ml, case.max_parts, case.table[order])
    e = engine_for(mixed)
    check(e, mixed)
    check(e, mixed, TS.MAX_PARTS)
    e.close()


def test_chunks_and_slices():
    """level_size = [65536, 512, 1]: the device holds the tables of 84 shapes at a time and the batch has 200, so
    three chunks; at max_parts 1024 a slice holds 8172 picks and the batch has 9000."""
    n, sizes = 1025, [65536, 512, 1]
    assert (64 << 20) // (12 * sum(sizes)) == 84 and (64 << 20) // (8 * 1024 + 20) == 8172
    inv = synth.make_inventory(n, 7)
    ids = (np.arange(n) * 63).astype(np.int32)
    parent = np.concatenate([np.arange(65536) // 128, np.zeros(512)]).astype(np.int32)
    S, C = 200, 45
    s_req = np.array([[100 * (j + 1), G.GiB, 0, 0] for j in range(S)], dtype=np.int64)
    c_slots, _ = DC.tables_of(G.capacity_matrix(inv.residual(), inv.labels, s_req, None), np.arange(n), n)
    leaf = np.zeros((S, 65536), dtype=np.int64)
    leaf[:, ids] = c_slots                                  # small integers: int64 sums are exact
    block = leaf.reshape(S, 512, 128).sum(axis=2)
    tab = np.concatenate([leaf, block, block.sum(axis=1, keepdims=True)], axis=1)
    np.testing.assert_array_equal(TC.rollup(leaf[[0, 199]], sizes, parent), tab[[0, 199]])
    shape = np.repeat(np.arange(S), C)
    top = tab[:, -1][shape]
    k = np.tile(np.arange(1, C + 1), S)
    count = np.where(k <= 34, k, np.maximum(1, (top + 1) * (k - 34) // 11)).astype(np.int32)   # most gangs small, a few up to none
    J = S * C
    order = np.random.default_rng(6).permutation(J)         # a slice's picks come from every chunk
    shape, count = shape[order], count[order]
    max_level = (np.arange(J) % 4 != 0).astype(np.int32) * 2
    picks = len(np.unique(np.stack([shape, count, max_level]), axis=1).T)
    assert picks > 8172, picks
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, ids)
    before = e.read_residuals()
    got = e.gang_split_tree(s_req[shape], None, count, max_level, sizes, parent, TS.MAX_PARTS)
    want = TS.split_wide(tab, shape, count, sizes, parent, max_level, TS.MAX_PARTS)
    TS.same(got, want, "three chunks, two slices")
    assert (want.parts > 100).any() and (want.parts == 0).any() and (want.parts == 1).any()
    kids = TS.children(sizes, parent)
    for j in (0, 1, 5000, J - 1):                           # the wide checker is the plain one
        r = TS.split_row(tab[shape[j]], int(count[j]), sizes, kids, int(max_level[j]))
        assert (r[0], r[1], r[2], r[4]) == (want.level[j], want.domain[j], want.parts[j], want.spread[j].tolist())
    small = e.gang_split_tree(s_req[shape], None, count, max_level, sizes, parent, 16)
    TS.same(small, TS.split_wide(tab, shape, count, sizes, parent, max_level, 16), "three chunks, one slice")
    np.testing.assert_array_equal(e.read_residuals(), before)
    e.close()


def raw_call(e, case, max_parts, outs, count="case", max_level="case", sizes=None, parent="case", req=None, n_jobs=None):
    sizes = np.ascontiguousarray(case.sizes if sizes is None else sizes, dtype=np.int32)
    parent = case.parent if isinstance(parent, str) else parent
    parent = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
    count = case.count if isinstance(count, str) else count
    max_level = case.max_level if isinstance(max_level, str) else max_level
    req = case.req if req is None else req
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    return e.lib.pe_gang_split_tree(e.h, req.shape[0] if n_jobs is None else n_jobs, ptr(req), ptr(case.need), ptr(count),
                                    ptr(max_level), len(sizes), sizes.ctypes.data, ptr(parent), max_parts,
                                    *[ptr(o) for o in outs])


def test_optional_outputs():
    """Each output alone, each one NULL in turn, all and none."""
    case = TS.named_case("racks32", 1025)
    e = engine_for(case)
    mp = case.max_parts
    full = e.gang_split_tree(case.req, case.need, case.count, case.max_level, case.sizes, case.parent, mp)
    TS.same(full, case.want())
    masks = [tuple(k == i for k in range(6)) for i in range(6)] + [tuple(k != i for k in range(6)) for i in range(6)]
    for on in masks + [(True,) * 6, (False,) * 6]:
        outs = [np.full(getattr(full, f).shape, -7, dtype=np.int32) if on[k] else None for k, f in enumerate(FIELDS)]
        assert raw_call(e, case, mp, outs) == _abi.PE_OK, on
        for k, f in enumerate(FIELDS):
            if on[k]:
                np.testing.assert_array_equal(outs[k], getattr(full, f), err_msg=str((on, f)))
    e.close()


def test_parts_are_placed():
    """The parts of a job, each as a one-group job in its leaf at level 0, in one pe_place_greedy_domains call
    on a fresh inventory: all placed, pod by pod on nodes of the part's leaf."""
    for name, n in (("racks32", 257), ("four", 257), ("permuted", 257)):
        case = TS.named_case(name, n)
        e = engine_for(case)
        got = e.gang_split_tree(case.req, case.need, case.count, case.max_level, case.sizes, case.parent, TS.MAX_PARTS)
        e.close()
        p = engine_for(case)
        placed = 0
        for j in np.flatnonzero(got.parts >= 1):
            k = int(got.parts[j])
            leaves, pods = got.part_domain[j, :k], got.part_pods[j, :k]
            assert pods.sum() == case.count[j]
            p.reset_residuals()
            pod_node, status = p.place_greedy_domains(np.arange(k + 1, dtype=np.int32), np.zeros(k, dtype=np.int32), pods,
                                                      np.tile(case.req[j], (k, 1)), np.full(k, case.need[j], dtype=np.uint32),
                                                      leaves, 0, case.sizes, case.parent)
            assert (status == _abi.PE_JOB_PLACED).all(), (name, j)
            np.testing.assert_array_equal(case.island[pod_node], np.repeat(leaves, pods))
            placed += k
        assert placed > 50
        p.close()


def test_state_is_untouched():
    """A context walked through a staged fit batch, the call, a placement, a node update, a reset and a reload,
    beside an engine that never made the call: the same residuals, fit masks, statistics and placements."""
    case = TS.named_case("racks32", 1025)
    a, b = engine_for(case), engine_for(case)
    f_req, f_need = synth.make_fit_jobs(200, 7)
    jobs = synth.make_jobs(60, 7, "mixed")

    def split(e):
        got = e.gang_split_tree(case.req, case.need, case.count, case.max_level, case.sizes, case.parent, case.max_parts)
        lab = synth.island_labels(e_labels, e_island)
        tab = TC.tables(e.read_residuals(), lab, e_island, case.req, case.need, case.sizes, case.parent)[0]
        TS.same(got, TS.split(tab, case.count, case.sizes, case.parent, case.max_level, case.max_parts))
        return got

    def both(f):
        ra, rb = f(a), f(b)
        for u, v in zip(ra if isinstance(ra, tuple) else (ra,), rb if isinstance(rb, tuple) else (rb,)):
            np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(a.read_residuals(), b.read_residuals())
        sa, sb = a.stats(), b.stats()
        assert {k: v for k, v in sa.items() if not k.endswith("_ms")} == {k: v for k, v in sb.items() if not k.endswith("_ms")}

    e_labels, e_island = case.labels.copy(), case.island.copy()
    for x in (a, b):
        x.jobs_upload(f_req, f_need)
        x.fit_mask_run()
    first = split(a)
    both(lambda x: x.fit_counts())
    both(lambda x: x.fit_mask_rows(0, 200))
    both(lambda x: x.place_batch(jobs))
    second = split(a)
    assert (second.parts != first.parts).any() or (second.part_pods != first.part_pods).any()
    slot = 7
    for x in (a, b):
        x.update_nodes([slot], [_abi.PE_NODE_SET], case.cap[:, 3][None], case.used[:, 3][None], case.labels[3:4],
                       [int(case.island[-1])])
    e_labels[slot], e_island[slot] = case.labels[3], case.island[-1]
    split(a)
    both(lambda x: (x.fit_mask_run(), x.fit_counts())[1])
    for x in (a, b):
        x.reset_residuals()
    split(a)
    both(lambda x: x.place_batch(jobs))
    other = TS.named_case("permuted", 257)
    for x in (a, b):
        x.load_nodes(other.cap, other.used, other.labels, other.island)
    check(a, other)
    both(lambda x: x.place_batch(jobs))
    a.close()
    b.close()


def test_alternation_with_the_capacity_calls():
    """The split between the three capacity calls on one context, in both orders: every answer is that of an
    engine that made only that call."""
    case = TS.named_case("four", 1025)
    other = TS.fan_case(65, "zero")
    e, ref = engine_for(case), engine_for(case)
    cnt = case.count

    def calls(x):
        return [lambda: x.gang_capacity(case.req, case.need),
                lambda: x.gang_capacity_domains(case.req, case.need, cnt, case.sizes[0]),
                lambda: x.gang_capacity_tree(case.req, case.need, cnt, case.max_level, case.sizes, case.parent),
                lambda: x.gang_capacity_tree(case.req[:7], case.need[:7], cnt[:7], None, case.sizes[:1], None, tables=False)]

    want = [c() for c in calls(ref)]
    ref.close()
    for k, c in enumerate(calls(e) + calls(e)[::-1]):
        check(e, case, (case.max_parts, TS.MAX_PARTS, 1)[k % 3])
        got = c()
        for u, v in zip(got, want[k] if k < 4 else want[7 - k]):
            assert (u is None) == (v is None)
            if u is not None:
                np.testing.assert_array_equal(u, v)
    check(e, case)
    e.load_nodes(other.cap, other.used, other.labels, other.island)
    check(e, other)
    e.close()


def test_errors():
    case = TS.named_case("racks32", 1025)
    J, L, mp = len(case.count), len(case.sizes), case.max_parts
    e = engine_for(case)

    def outputs(width=mp):
        return [np.full(J, -7, dtype=np.int32), np.full(J, -7, dtype=np.int32), np.full(J, -7, dtype=np.int32),
                np.full((J, width), -7, dtype=np.int32), np.full((J, width), -7, dtype=np.int32),
                np.full((J, L), -7, dtype=np.int32)]

    def refused(text, max_parts=mp, **kw):
        """PE_EINVAL with `text` in the message, and no output written."""
        outs = outputs()
        assert raw_call(e, case, max_parts, outs, **kw) == _abi.PE_EINVAL, text
        msg = e.lib.pe_last_error(e.h).decode()
        assert text in msg, msg
        for o in outs:
            assert (o == -7).all(), text

    for v in (0, -1, _abi.PE_MAX_SPLIT_PARTS + 1, 2**31 - 1):
        refused("max_parts outside [1, PE_MAX_SPLIT_PARTS]", max_parts=v)
    bad = case.req.copy()
    bad[5, 2] = -1
    refused("index 22", req=bad)
    zero = case.count.copy()
    zero[7], zero[11] = 0, -3
    refused("count: value below 1 at index 7", count=zero)
    refused("count is NULL", count=None)
    for v in (L, -1, 2**31 - 1):
        ml = case.max_level.copy()
        ml[4] = v
        refused("max_level: value outside [0, n_levels) at index 4", max_level=ml)
    for n in (0, 5):
        refused("n_levels", sizes=[4] * n, parent=np.zeros(16, dtype=np.int32))
    for k, v in ((0, 0), (1, 0), (2, -1), (1, _abi.PE_MAX_DOMAINS + 1)):
        s = list(case.sizes)
        s[k] = v
        refused(f"level_size: value outside [1, PE_MAX_DOMAINS] at index {k}", sizes=s)
    for at, v in ((3, case.sizes[1]), (5, -2), (case.sizes[0] + 2, 1)):
        p = np.array(case.parent, dtype=np.int32)
        p[at] = v
        refused(f"parent: value outside [-1, size of the level above) at index {at}", parent=p)
    refused("parent is NULL", parent=None)
    refused("n_jobs < 0", n_jobs=-1)
    # no jobs; the Python handle raises what the engine returns
    assert raw_call(e, case, mp, [None] * 6, n_jobs=0) == _abi.PE_OK
    none = e.gang_split_tree(np.zeros((0, 4), dtype=np.int64), None, np.zeros(0, dtype=np.int32), None, case.sizes,
                             case.parent, 4)
    assert none.parts.shape == (0,) and none.part_domain.shape == (0, 4) and none.spread.shape == (0, L)
    with pytest.raises(PlacementError) as ei:
        e.gang_split_tree(case.req, case.need, case.count, None, case.sizes, case.parent, 0)
    assert ei.value.code == _abi.PE_EINVAL and "max_parts" in str(ei.value)
    e.close()
    fresh = Engine(0)
    with pytest.raises(PlacementError) as ei:
        fresh.gang_split_tree(case.req, case.need, case.count, None, case.sizes, case.parent, mp)
    assert ei.value.code == _abi.PE_ESTATE
    # an inventory of no nodes: -1 / 0 everywhere, whatever the arrays held
    fresh.load_nodes(np.zeros((4, 0), dtype=np.int64), np.zeros((4, 0), dtype=np.int64))
    outs = outputs()
    assert raw_call(fresh, case, mp, outs) == _abi.PE_OK
    assert (outs[0] == -1).all() and (outs[1] == -1).all() and not outs[2].any()
    assert (outs[3] == -1).all() and not outs[4].any() and not outs[5].any()
    fresh.close()
    # a sharded context: the selection needs the global table
    for r in range(2):
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(case.cap, case.used, case.labels, case.island)
        outs = outputs()
        assert raw_call(s, case, mp, outs) == _abi.PE_EINVAL
        assert "shard" in s.lib.pe_last_error(s.h).decode() and all((o == -7).all() for o in outs)
        s.close()
