"""pe_gang_slice_tree on the GPU against the Python-integer checker (tests/tree_slices.py): every cell of every
output of every job compared, nothing sampled, and the residuals before and after."""
import numpy as np
import pytest

import domain_placement as DP
import gang_capacity as G
import tree_capacity as TC
import tree_slices as SL
import tree_split as TS
from placement import Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

OUT = ("level", "domain", "domain_units", "parts", "part_domain", "part_pods", "spread")


def engine_for(case):
    e = Engine(0)
    e.load_nodes(case.cap, case.used, case.labels, case.island)
    return e


def call(e, case, mp, ml):
    return e.gang_slice_tree(case.req, case.need, case.count, case.z, case.sl, ml, case.sizes, case.parent, mp)


def check(e, case, max_parts=None, max_level="case"):
    """One call against the checker, the residuals untouched; returns the engine's answer."""
    mp = case.max_parts if max_parts is None else max_parts
    ml = case.max_level if isinstance(max_level, str) else max_level
    before = e.read_residuals()
    got = call(e, case, mp, ml)
    np.testing.assert_array_equal(e.read_residuals(), before)
    SL.same(SL.of_engine(got), case.want(max_parts=mp, max_level=ml), f"max_parts {mp}")
    return got


def all_of(name, n, strict=True):
    """Every (z, sl) case of a named tree as one batch: each job with its own slice size and level."""
    return SL.merged([c for c, _ in SL.named_cases(name, n, strict=strict).values()])


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n_nodes", [1, 255, 257, 1025])
def test_sizes_and_trees(n_nodes, name):
    case = all_of(name, n_nodes, strict=n_nodes > 255)
    e = engine_for(case)
    got = check(e, case)
    check(e, case, SL.MAX_PARTS)
    # max_level at m for every job, and NULL
    check(e, case, SL.MAX_PARTS, np.maximum(case.sl, 0))
    check(e, case, 1, None)
    if n_nodes > 255 and len(case.sizes) > 1:
        assert (got.parts > 1).any() and (got.parts == SL.TOO_MANY).any() and (got.parts == 0).any()
    # NULL slice_size and slice_level: slices of one pod at level 0
    plain = e.gang_slice_tree(case.req, case.need, case.count, None, None, case.max_level, case.sizes, case.parent, case.max_parts)
    TS.same(plain, e.gang_split_tree(case.req, case.need, case.count, case.max_level, case.sizes, case.parent, case.max_parts))
    e.close()


@pytest.mark.parametrize("kind", TS.FAN_KINDS)
@pytest.mark.parametrize("fan_in", [1, 63, 64, 65, 200])
def test_fan_in_boundaries(fan_in, kind):
    case = SL.fan_case(fan_in, kind)
    e = engine_for(case)
    check(e, case)
    check(e, case, SL.MAX_PARTS)
    e.close()


@pytest.mark.parametrize("trap", SL.TRAPS, ids=[t[0] for t in SL.TRAPS])
def test_traps(trap):
    name, _, _, _, _, _, _, _, level, domain, units, parts, spread = trap
    case = SL.trap_case(trap)
    e = engine_for(case)
    got = check(e, case)
    n = len(parts)
    assert (got.level[0], got.domain[0], got.domain_units[0], got.parts[0]) == (level, domain, units, n)
    assert got.spread[0].tolist() == spread
    assert list(zip(got.part_domain[0, :n].tolist(), got.part_pods[0, :n].tolist())) == parts
    e.close()


def test_extreme_slice_sizes():
    """A slice larger than any node or domain holds, and a shape that asks for nothing (PE_CAP_MAX pods per node)
    in slices of 2^31 - 1: one unit per node at node level, one per node of the rack at level 0."""
    base = SL.named_cases("racks32", 257)[(1, 0)][0]
    big = 2**31 - 1
    reqs = np.concatenate([base.req[:1], np.zeros((1, 4), dtype=np.int64)])
    lab = synth.island_labels(base.labels, base.island)
    jobs = [(0, 1, 1 << 24, sl, None) for sl in range(-1, 3)] + [(1, 1, big, sl, None) for sl in range(-1, 3)]
    case = SL.build(base.cap, base.used, base.labels, lab, base.island, base.sizes, base.parent, reqs,
                    np.zeros(2, dtype=np.uint32), jobs, 4)
    assert case.rows[4][0] == case.rows[5][0] == case.table[4][0] // big >= 1
    e = engine_for(case)
    got = check(e, case)
    assert (got.parts[:4] == 0).all() and (got.parts[4:] == 1).all() and (got.part_pods[4:, 0] == big).all()
    e.close()


def test_max_parts_boundary():
    """65 one-unit leaves (3 free GPUs, slices of 2): 65 slices need exactly 65 parts."""
    cap, used, labels, island = TS.leaf_inventory([3] * 65)
    sizes, parent = [65, 1], np.zeros(65, dtype=np.int32)
    jobs = [(0, u, 2, sl, None) for sl in (SL.NODE, 0) for u in (65, 64, 2, 1, 66)]
    case = SL.build(cap, used, labels, labels | np.uint32(1 << 31), island, sizes, parent, [TS.GPU_REQ], None, jobs, 65)
    e = engine_for(case)
    for mp, parts in ((1, [-1, -1, -1, 1, 0]), (64, [-1, 64, 2, 1, 0]), (65, [65, 64, 2, 1, 0]), (1024, [65, 64, 2, 1, 0])):
        got = check(e, case, mp)
        assert got.parts.tolist() == parts * 2 and got.part_domain.shape == (10, mp)
    assert got.part_domain[0, :65].tolist() == list(range(65)) and (got.part_pods[0, :65] == 2).all()
    e.close()


def test_recurring_rows():
    """The rows are the distinct (shape, z, sl), the picks the distinct (row, units, max_level): jobs that recur out of
    order under other levels, and exact repeats."""
    case = all_of("four", 1025)
    rng = np.random.default_rng(5)
    J = len(case.count)
    order = rng.permutation(np.concatenate([np.arange(J), np.arange(J)[::3]]))[:600]
    ml = np.maximum(rng.integers(0, len(case.sizes), len(order)), case.sl[order]).astype(np.int32)
    mixed = SL.Case(case.cap, case.used, case.labels, case.island, case.sizes, case.parent, case.req[order], case.need[order],
                    case.count[order], case.z[order], case.sl[order], ml, case.max_parts, [case.rows[j] for j in order],
                    case.table[order])
    e = engine_for(mixed)
    check(e, mixed)
    check(e, mixed, SL.MAX_PARTS)
    e.close()


def test_chunks_and_slices():
    """level_size = [65536, 512, 1]: the device holds the tables of 127 rows at a time and the batch has 140, so two
    chunks; at max_parts 1024 a slice holds 8172 picks and the batch has more.  Node-level and level-0 rows: the
    descent is tree_split's on the unit table, the parts times z."""
    n, sizes = 1025, [65536, 512, 1]
    assert (64 << 20) // (8 * sum(sizes)) == 127 and (64 << 20) // (8 * 1024 + 20) == 8172
    inv = synth.make_inventory(n, 7)
    ids = (np.arange(n) * 63).astype(np.int32)
    parent = np.concatenate([np.arange(65536) // 128, np.zeros(512)]).astype(np.int32)
    req = np.array([[100, G.GiB, 0, 0]], dtype=np.int64)
    caps = G.capacity_matrix(inv.residual(), inv.labels, req, None)[0].astype(np.int64)   # one node per used leaf
    R, C = 140, 60
    zs, sls = np.arange(R) // 2 + 2, np.arange(R) % 2 - 1           # z = 2 .. 71 at node level and at level 0
    leaf = np.zeros((R, 65536), dtype=np.int64)
    leaf[:, ids] = caps[None, :] // zs[:, None]
    block = leaf.reshape(R, 512, 128).sum(axis=2)
    tab = np.concatenate([leaf, block, block.sum(axis=1, keepdims=True)], axis=1)
    row = np.repeat(np.arange(R), C)
    top = tab[:, -1][row]
    k = np.tile(np.arange(1, C + 1), R)
    units = np.where(k <= 48, k, np.maximum(1, (top + 1) * (k - 48) // 11)).astype(np.int64)
    J = R * C
    order = np.random.default_rng(6).permutation(J)
    row, units = row[order], units[order]
    max_level = (np.arange(J) % 4 != 0).astype(np.int32) * 2
    assert len(np.unique(np.stack([row, units, max_level]), axis=1).T) > 8172
    z, sl = zs[row].astype(np.int32), sls[row].astype(np.int32)
    count = (units * z).astype(np.int32)
    assert (units * z < 2**31).all()
    e = Engine(0)
    e.load_nodes(inv.cap, inv.used, inv.labels, ids)
    before = e.read_residuals()
    got = e.gang_slice_tree(np.repeat(req, J, axis=0), None, count, z, sl, max_level, sizes, parent, SL.MAX_PARTS)
    want = TS.split_wide(tab, row, units, sizes, parent, max_level, SL.MAX_PARTS)
    want.part_pods = want.part_pods * z[:, None]
    TS.same(got, want, "two chunks, two slices")
    lvl = np.maximum(want.level, 0)
    col = np.where(lvl == 0, 0, np.where(lvl == 1, 65536, 65536 + 512)) + np.maximum(want.domain, 0)
    np.testing.assert_array_equal(got.domain_units, np.where(want.level >= 0, tab[row, col], 0))
    assert (want.parts == 1).any() and (want.parts == 0).any() and (want.parts > 8).any()
    np.testing.assert_array_equal(e.read_residuals(), before)
    e.close()


def raw_call(e, case, max_parts, outs, n_jobs=None, sizes=None, parent="case", **kw):
    sizes = np.ascontiguousarray(case.sizes if sizes is None else sizes, dtype=np.int32)
    parent = case.parent if isinstance(parent, str) else parent
    parent = None if parent is None else np.ascontiguousarray(parent, dtype=np.int32)
    a = {f: kw.get(f, getattr(case, f)) for f in ("req", "need", "count", "z", "sl", "max_level")}
    ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    return e.lib.pe_gang_slice_tree(e.h, a["req"].shape[0] if n_jobs is None else n_jobs, ptr(a["req"]), ptr(a["need"]),
                                    ptr(a["count"]), ptr(a["z"]), ptr(a["sl"]), ptr(a["max_level"]), len(sizes),
                                    sizes.ctypes.data, ptr(parent), max_parts, *[ptr(o) for o in outs])


def filled(full):
    return [np.full(getattr(full, f).shape, -7, dtype=getattr(full, f).dtype) for f in OUT]


def test_optional_outputs():
    """Each output alone, each one NULL in turn, all and none."""
    case = all_of("racks32", 257)
    e = engine_for(case)
    mp = case.max_parts
    full = check(e, case)
    masks = [tuple(k == i for k in range(7)) for i in range(7)] + [tuple(k != i for k in range(7)) for i in range(7)]
    for on in masks + [(True,) * 7, (False,) * 7]:
        outs = [o if on[k] else None for k, o in enumerate(filled(full))]
        assert raw_call(e, case, mp, outs) == _abi.PE_OK, on
        for k, f in enumerate(OUT):
            if on[k]:
                np.testing.assert_array_equal(outs[k], getattr(full, f), err_msg=str((on, f)))
    e.close()


@pytest.mark.parametrize("name", ["racks32", "four", "permuted"])
def test_parts_are_placed(name):
    """The parts of a job in one pe_place_greedy_domains call on a fresh inventory, all placed: with sl >= 0 each part
    a one-group job in its leaf, at node level part (leaf, a * z) one job of a island groups of z pods."""
    case = all_of(name, 257)
    e = engine_for(case)
    got = call(e, case, SL.MAX_PARTS, case.max_level)
    placed = {True: 0, False: 0}
    for j in np.flatnonzero((got.parts >= 1) & (case.z > 1)):
        k, z, node = int(got.parts[j]), int(case.z[j]), case.sl[j] == SL.NODE
        leaves, pods = got.part_domain[j, :k], got.part_pods[j, :k]
        assert pods.sum() == case.count[j]
        groups = pods // z if node else np.ones(k, dtype=np.int32)
        G_ = int(groups.sum())
        need = int(case.need[j]) | (DP.ISLAND if node else 0)
        e.reset_residuals()
        pod_node, status = e.place_greedy_domains(np.concatenate([[0], np.cumsum(groups)]).astype(np.int32),
                                                  np.zeros(k, dtype=np.int32),
                                                  np.full(G_, z, dtype=np.int32) if node else pods,
                                                  np.tile(case.req[j], (G_, 1)), np.full(G_, need, dtype=np.uint32),
                                                  leaves, 0, case.sizes, case.parent)
        assert (status == _abi.PE_JOB_PLACED).all(), (name, j)
        np.testing.assert_array_equal(case.island[pod_node], np.repeat(leaves, pods))
        if node:   # every island group on one node
            assert all(len(set(g)) == 1 for g in pod_node.reshape(-1, z).tolist())
        placed[bool(node)] += k
    assert placed[True] > 10 and placed[False] > 10
    e.close()


def test_state_is_untouched():
    """A context walked through a staged fit batch, the call, a placement, a node update, a reset and a reload,
    beside an engine that never made the call: the same residuals, fit masks, statistics and placements."""
    case = all_of("racks32", 257)
    a, b = engine_for(case), engine_for(case)
    f_req, f_need = synth.make_fit_jobs(200, 7)
    jobs = synth.make_jobs(60, 7, "mixed")
    shapes = np.unique(np.concatenate([case.req, case.need[:, None].astype(np.int64)], axis=1), axis=0, return_inverse=True)
    s_req, s_need, s_of = shapes[0][:, :4], shapes[0][:, 4].astype(np.uint32), shapes[1].reshape(-1)

    def ask(e):
        got = call(e, case, case.max_parts, case.max_level)
        lab = synth.island_labels(e_labels, e_island)
        now = SL.build(case.cap, case.cap - e.read_residuals(), e_labels, lab, e_island, case.sizes, case.parent, s_req, s_need,
                       [(int(s_of[j]), int(case.count[j] // case.z[j]), int(case.z[j]), int(case.sl[j]), int(case.max_level[j]))
                        for j in range(len(case.count))], case.max_parts)
        SL.same(SL.of_engine(got), now.want())
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
    first = ask(a)
    both(lambda x: x.fit_counts())
    both(lambda x: x.fit_mask_rows(0, 200))
    both(lambda x: x.place_batch(jobs))
    second = ask(a)
    assert (second.parts != first.parts).any() or (second.part_pods != first.part_pods).any()
    slot = 7
    for x in (a, b):
        x.update_nodes([slot], [_abi.PE_NODE_SET], case.cap[:, 3][None], case.used[:, 3][None], case.labels[3:4],
                       [int(case.island[-1])])
    e_labels[slot], e_island[slot] = case.labels[3], case.island[-1]
    cap7 = case.cap.copy()
    cap7[:, slot] = case.cap[:, 3]
    case.cap = cap7      # (a copy: the shared case keeps its own)
    ask(a)
    both(lambda x: (x.fit_mask_run(), x.fit_counts())[1])
    for x in (a, b):
        x.reset_residuals()
    ask(a)
    both(lambda x: x.place_batch(jobs))
    other = all_of("permuted", 257)
    for x in (a, b):
        x.load_nodes(other.cap, other.used, other.labels, other.island)
    check(a, other)
    both(lambda x: x.place_batch(jobs))
    a.close()
    b.close()


def test_alternation_with_the_capacity_calls():
    """The call between the three capacity calls and pe_gang_split_tree on one context, in both orders: every answer
    is that of an engine that made only that call."""
    case = all_of("four", 257)
    other = SL.fan_case(65, "zero")
    e, ref = engine_for(case), engine_for(case)
    cnt = case.count

    def calls(x):
        return [lambda: x.gang_capacity(case.req, case.need),
                lambda: x.gang_capacity_domains(case.req, case.need, cnt, case.sizes[0]),
                lambda: x.gang_capacity_tree(case.req, case.need, cnt, case.max_level, case.sizes, case.parent),
                lambda: x.gang_split_tree(case.req, case.need, cnt, case.max_level, case.sizes, case.parent, 16)]

    want = [c() for c in calls(ref)]
    ref.close()
    for k, c in enumerate(calls(e) + calls(e)[::-1]):
        check(e, case, (case.max_parts, SL.MAX_PARTS, 1)[k % 3])
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
    case = all_of("racks32", 257)
    J, L, mp = len(case.count), len(case.sizes), case.max_parts
    e = engine_for(case)
    full = call(e, case, mp, case.max_level)

    def refused(text, max_parts=mp, eng=e, **kw):
        """PE_EINVAL with `text` in the message, and no output written."""
        outs = filled(full)
        assert raw_call(eng, case, max_parts, outs, **kw) == _abi.PE_EINVAL, text
        msg = eng.lib.pe_last_error(eng.h).decode()
        assert text in msg, msg
        for o in outs:
            assert (o == -7).all(), text

    def with_(field, at, v):
        a = getattr(case, field).copy()
        a[at] = v
        return {field: a}

    for v in (0, -1, _abi.PE_MAX_SPLIT_PARTS + 1):
        refused("max_parts outside [1, PE_MAX_SPLIT_PARTS]", max_parts=v)
    bad = case.req.copy()
    bad[5, 2] = -1
    refused("index 22", req=bad)
    refused("count: value below 1 at index 7", **with_("count", [7, 11], [0, -3]))
    refused("count is NULL", count=None)
    for v in (L, -1, 2**31 - 1):
        refused("max_level: value outside [0, n_levels) at index 4", **with_("max_level", 4, v))
    for v in (0, -1, -2**31):
        refused("slice_size: value below 1 at index 9", **with_("z", [9, 30], v))
    at = int(np.flatnonzero(case.z == 8)[2])
    refused(f"count: not a multiple of slice_size at index {at}", **with_("count", at, int(case.count[at]) + 1))
    for v in (-2, L, 2**31 - 1):
        refused("slice_level: value outside [PE_SLICE_NODE, n_levels) at index 6", **with_("sl", [6, 8], v))
    at = int(np.flatnonzero(case.sl == 2)[1])
    refused(f"max_level: value below max(slice_level, 0) at index {at}", **with_("max_level", at, 1))
    low = np.ones(J, dtype=np.int32)
    refused(f"max_level: value below max(slice_level, 0) at index {int(np.flatnonzero(case.sl == 2)[0])}", max_level=low)
    for n in (0, 5):
        refused("n_levels", sizes=[4] * n, parent=np.zeros(16, dtype=np.int32))
    s = list(case.sizes)
    s[1] = 0
    refused("level_size: value outside [1, PE_MAX_DOMAINS] at index 1", sizes=s)
    p = np.array(case.parent, dtype=np.int32)
    p[3] = case.sizes[1]
    refused("parent: value outside [-1, size of the level above) at index 3", parent=p)
    refused("parent is NULL", parent=None)
    refused("n_jobs < 0", n_jobs=-1)
    # a defaulted max_level is the top level: nothing to refuse; no jobs
    assert raw_call(e, case, mp, filled(full), max_level=None) == _abi.PE_OK
    assert raw_call(e, case, mp, [None] * 7, n_jobs=0) == _abi.PE_OK
    none = e.gang_slice_tree(np.zeros((0, 4), dtype=np.int64), None, np.zeros(0, dtype=np.int32), level_size=case.sizes,
                             parent=case.parent, max_parts=4)
    assert none.parts.shape == (0,) and none.part_domain.shape == (0, 4) and none.domain_units.shape == (0,)
    with pytest.raises(PlacementError) as ei:
        e.gang_slice_tree(case.req, case.need, case.count, np.zeros(J, dtype=np.int32), None, None, case.sizes, case.parent)
    assert ei.value.code == _abi.PE_EINVAL and "slice_size" in str(ei.value)
    e.close()
    fresh = Engine(0)
    with pytest.raises(PlacementError) as ei:
        call(fresh, case, mp, case.max_level)
    assert ei.value.code == _abi.PE_ESTATE
    # an inventory of no nodes: -1 / 0 everywhere, whatever the arrays held
    fresh.load_nodes(np.zeros((4, 0), dtype=np.int64), np.zeros((4, 0), dtype=np.int64))
    outs = filled(full)
    assert raw_call(fresh, case, mp, outs) == _abi.PE_OK
    assert (outs[0] == -1).all() and (outs[1] == -1).all() and not outs[2].any() and not outs[3].any()
    assert (outs[4] == -1).all() and not outs[5].any() and not outs[6].any()
    refused("slice_size: value below 1 at index 9", eng=fresh, **with_("z", 9, 0))
    fresh.close()
    # a sharded context: node-level units cannot be had from the shards' tables
    for r in range(2):
        s = Engine(0, rank=r, world_size=2, exchange=lambda b: b * 2)
        s.load_nodes(case.cap, case.used, case.labels, case.island)
        outs = filled(full)
        assert raw_call(s, case, mp, outs) == _abi.PE_EINVAL
        assert "shard" in s.lib.pe_last_error(s.h).decode() and all((o == -7).all() for o in outs)
        s.close()
