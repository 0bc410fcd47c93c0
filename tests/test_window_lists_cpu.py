"""window_lists.py on the host model alone: the script of test_gpu_window_lists.py yields lists of every kind -- full
with a real limit, short with the bound as limit, empty, taken with saturating nodes in the overlay -- at every topk,
node count and inventory kind, and its calls are one window each; scan_bound against a plain loop; read_dump on a
file written here in the engine's layout.

EDGE_CONFIGS, on the model alone: their inventories and requests reach what they are named for -- a walk emulated
with less than the kernel's slack of 2 is wrong on them (and on none of CONFIGS' lists), pairs with 0, 1 and 2 borrows
and keys that carry into the high word exist, rare_borrow's K-th key lies past the in-walk compaction threshold,
the thresholds nodes fall on both sides of every line of node_prep, and the two restatements of the key agree there."""
import functools
import os
import struct

import numpy as np

import scan_emulator
import window_lists as wl
from placement import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configurations_cover_every_topk_node_count_and_kind():
    assert {c.topk for c in wl.CONFIGS} == set(wl.TOPK)
    assert {c.n for c in wl.CONFIGS} == set(wl.NODES)
    assert {c.kind for c in wl.CONFIGS} == set(wl.KINDS)
    assert wl.Config(1023, 5000, "random") in wl.CONFIGS and wl.Config(1023, 2049, "identical") in wl.CONFIGS
    for cfg in wl.CONFIGS:
        places = [st.arg for st in wl.script(cfg) if st.op == "place"]
        assert len(places) == 5 and any(st.op == "update" for st in wl.script(cfg))
        for b in places:   # one window holds the whole call
            assert len(b.group_count) <= wl.WINDOW_GROUPS and int(b.group_count.sum()) <= wl.WINDOW_PODS
            assert len(wl.first_window(b)) == int((b.group_count > 0).sum())


def test_the_model_alone_yields_lists_of_every_kind():
    for scan in (False, True):
        t = wl.totals(scan)
        print("scan" if scan else "walk", t)
        assert t.lists >= 400 and t.full >= 100 and t.short >= 50 and t.empty >= 20 and t.overlay >= 80, t
    # and per configuration: the largest lists are full where the inventory holds more nodes than topk
    assert wl.model_counts(wl.Config(1023, 5000, "random"), False).full >= 10
    assert wl.model_counts(wl.Config(1023, 2049, "identical"), False).full >= 10
    assert wl.model_counts(wl.Config(1023, 1023, "saturating"), False).short >= 10
    assert wl.model_counts(wl.Config(1, 1, "identical"), False).full == 0


def test_scan_bound_is_the_smallest_second_best_key_of_a_lane():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 1024, 1025, 3000):
        k = rng.integers(1, 1 << 50, size=n, dtype=np.uint64)
        k[rng.random(n) < 0.5] = wl.NO_KEY
        best = wl.NO_KEY
        for w0 in range(0, n, 1024):
            for lane in range(64):
                mine = sorted(int(x) for x in k[w0 + lane:min(w0 + 1024, n):64])
                if len(mine) > 1:
                    best = min(best, mine[1])
        assert wl.scan_bound(k) == best, n
    assert wl.scan_bound(np.array([5, 6], dtype=np.uint64)) == wl.NO_KEY     # two lanes, one key each


def test_expected_lists_on_a_hand_made_inventory():
    res = np.array([[4000, 3000, 2000, 1000, 500], [8 << 30] * 5, [0] * 5, [0] * 5], dtype=np.int64)
    labels = np.zeros(5, np.uint32)
    b = synth.JobBatch(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3], np.int32),
                       np.array([[1000, 1 << 30, 0, 0]], np.int64), np.zeros(1, np.uint32), np.zeros(1, np.int8))
    k = scan_emulator.keys(res, labels, b.group_req[0], 0, 0)
    order = sorted(int(x) for x in k if x != scan_emulator.NO_KEY)
    assert [x & 0xFFFFFF for x in order] == [3, 2, 1, 0]            # the tightest fit first; node 4 does not fit
    assert wl.expected_lists(res, labels, b, [0], 2, False) == [(2, order[2], order[:2])]
    assert wl.expected_lists(res, labels, b, [0], 4, False) == [(4, wl.NO_KEY, order)]
    assert wl.expected_lists(res, labels, b, [0], 8, True) == [(4, wl.NO_KEY, order)]   # one key per lane: no bound


def test_read_dump_reads_the_engines_layout(tmp_path):
    J, G, stride = 2, 3, 4
    blob = b""
    lists = [(2, 7, 99, [10, 20]), (0, 7, wl.NO_KEY, []), (4, 7, 50, [1, 2, 3, 4])]
    for n, flags, limit, keys in lists:
        blob += struct.pack("<iiQ4Q", n, flags, limit, *(keys + [0] * (4 - n)))
    raw = struct.pack("<3q", J, G, stride) + bytes(4 * (J + 1) + 4 * J + 4 * G + 32 * G + 4 * G)
    raw += struct.pack("<q", 5) + bytes(5 * wl.NODE_STATE_BYTES)
    raw += struct.pack("<i3i", 3, 2, 0, 1) + blob + struct.pack("<i", 0)
    p = tmp_path / "d.bin"
    p.write_bytes(raw)
    assert wl.read_dump(str(p)) == (4, [2, 0, 1], lists, 0)


# ---------------------------------------------------------------- EDGE_CONFIGS: the key arithmetic at its edges

HDR = wl.walk_constants(os.path.join(ROOT, "training-operator_amd", "csrc", "pe_kernels.h"))
WALKED_KINDS = ("plateau", "staircase", "rare_borrow")


@functools.lru_cache(maxsize=None)
def states(cfg):
    return wl.first_window_states(cfg)


@functools.lru_cache(maxsize=None)
def wrong_lists(cfg):
    """(lists, wrong with slack 0, wrong with slack 1) of the emulated walk over the script's first windows; slack 2,
    the kernel's, must give expected_lists on every list."""
    lists, wrong = 0, [0, 0]
    for res, labels, b, groups in states(cfg):
        req = synth.scan_requests(b)
        want = wl.expected_lists(res, labels, b, groups, cfg.topk, False)
        for g, w in zip(groups, want):
            need = int(b.group_need[g])
            kw = dict(multi=HDR["WK_MULTI"], multi_after=HDR["WK_MULTI_AFTER"])
            assert wl.emulated_walk(res, labels, req[g], need, cfg.topk, 2, **kw)[0] == w, (cfg, g)
            for slack in (0, 1):
                wrong[slack] += wl.emulated_walk(res, labels, req[g], need, cfg.topk, slack, **kw)[0] != w
            lists += 1
    return lists, wrong[0], wrong[1]


def test_the_header_has_the_walk_constants_the_emulation_restates():
    assert HDR["WK_ROUND"] == 1024 and HDR["MG_CAP"] == 16384 and HDR["WK_MULTI"] >= 1 and HDR["WK_MULTI_AFTER"] >= 0


def test_edge_configurations_are_one_window_each():
    assert {c.kind for c in wl.EDGE_CONFIGS} == set(wl.EDGE_KINDS)
    assert not set(wl.EDGE_CONFIGS) & set(wl.CONFIGS) and not set(wl.EDGE_KINDS) & set(wl.KINDS)
    for cfg in wl.EDGE_CONFIGS:
        steps = wl.script(cfg)
        assert [st.op for st in steps] == [st.op for st in wl.script(wl.CONFIGS[0])]
        for st in steps:
            if st.op == "place":
                b = st.arg
                assert len(b.group_count) <= wl.WINDOW_GROUPS and int(b.group_count.sum()) <= wl.WINDOW_PODS
                assert len(wl.first_window(b)) == int((b.group_count > 0).sum())
                if cfg.kind == "rare_borrow":
                    assert ((b.group_req[:, 1] & wl.LO1) != 0).all() and ((b.group_req[:, 3] & wl.LO3) != 0).all()
            elif st.op == "update":     # the scatter's refresh of K(n) and the low parts is visible: odd low bits
                assert (st.arg[2][:, 1] & 1).all() and (st.arg[2][:, 3] & 1).all()
        inv = steps[0].arg
        assert inv.n == cfg.n and (inv.cap[2] == 8).all() == (cfg.kind != "thresholds")
        assert ((inv.labels & 0b11) == 0b11).all() and (inv.labels & synth.LABEL_ISLAND).all()


def test_a_walk_with_less_slack_is_wrong_on_the_edge_inventories_only():
    """The emulated walk (window_lists.emulated_walk) equals expected_lists with the kernel's slack of 2 on every
    list.  With slack 0 it is wrong on lists of every walked kind and with slack 1 on plateau and staircase lists,
    at one topk of the kind at least; on the inventories of CONFIGS slack 0 is wrong on none -- no list of theirs
    can tell.  rare_borrow and slack 1: its nodes borrow twice or never until the update step (the donor nodes are
    40 of 30 000), so the keys a slack of 1 miscounts -- one borrow -- do not exist in numbers that reach K + 1; it
    is the slack-0 and long-walk case and its slack-1 count is printed, not asserted."""
    per_kind = {k: [0, 0] for k in WALKED_KINDS}
    for cfg in wl.EDGE_CONFIGS:
        if cfg.kind in WALKED_KINDS:
            lists, w0, w1 = wrong_lists(cfg)
            print(cfg, "lists %d, wrong with slack 0 / 1 / 2: %d / %d / 0" % (lists, w0, w1))
            per_kind[cfg.kind][0] += w0
            per_kind[cfg.kind][1] += w1
    assert all(per_kind[k][0] > 0 for k in WALKED_KINDS), per_kind
    assert per_kind["plateau"][1] > 0 and per_kind["staircase"][1] > 0, per_kind
    for cfg in wl.CONFIGS:
        lists, w0, w1 = wrong_lists(cfg)
        assert lists > 0 and (w0, w1) == (0, 0), (cfg, w0, w1)


def pair_classes(cfg):
    """Over the first windows: the fitting (group, walkable node) pairs by borrow count, and those whose key carries
    across bit 32 when borrows << 24 leaves the low word: (score + borrows) & 0xFF < borrows."""
    by_borrows, carries = [0, 0, 0], 0
    for res, labels, b, groups in states(cfg):
        walkable = wl.node_class(res)[0] == 1
        req = synth.scan_requests(b)
        for g in groups:
            k = scan_emulator.keys(res, labels, req[g], int(b.group_need[g]), 0)
            fit = walkable & (k != scan_emulator.NO_KEY)
            q1, q3 = int(req[g][1]) & wl.LO1, int(req[g][3]) & wl.LO3
            bor = ((res[1] & wl.LO1) < q1).astype(np.uint64) + ((res[3] & wl.LO3) < q3).astype(np.uint64)
            score = k >> np.uint64(24)
            for n in range(3):
                by_borrows[n] += int((fit & (bor == n)).sum())
            carries += int((fit & (((score + bor) & np.uint64(0xFF)) < bor)).sum())
    return by_borrows, carries


def test_edge_configurations_reach_every_borrow_count_and_the_carry():
    for cfg in wl.EDGE_CONFIGS:
        by_borrows, carries = pair_classes(cfg)
        print(cfg, "fitting pairs with 0 / 1 / 2 borrows", by_borrows, "carrying into the high word", carries)
        if cfg.kind in ("plateau", "staircase"):
            assert min(by_borrows) > 0 and carries > 0, (cfg, by_borrows, carries)
        if cfg.kind == "staircase":     # every low score byte: for every fitting group some node's key carries
            assert carries >= 100, (cfg, carries)
        if cfg.kind == "rare_borrow":
            assert by_borrows[0] > 0 and by_borrows[2] > 0, (cfg, by_borrows)
    assert sum(pair_classes(c)[0][1] + pair_classes(c)[0][2] for c in wl.CONFIGS if c.kind != "saturating") == 0


def test_rare_borrow_walks_past_the_compaction_threshold():
    (cfg,) = [c for c in wl.EDGE_CONFIGS if c.kind == "rare_borrow"]
    room = HDR["MG_CAP"] - HDR["WK_MULTI"] * HDR["WK_ROUND"]
    res, labels, b, groups = states(cfg)[0]
    cls, S = wl.node_class(res)
    assert (cls == 1).all() and len(set(S.tolist())) == 1       # one plateau: sorted position = node id
    rare = np.nonzero((res[1] & wl.LO1) == 0)[0]
    assert np.array_equal(rare, np.arange(0, cfg.n, wl.RARE_EVERY)) and ((res[3][rare] & wl.LO3) == 0).all()
    assert len(rare) > cfg.topk and rare[cfg.topk - 1] > room and rare[cfg.topk] < cfg.n
    req = synth.scan_requests(b)
    long_walks = 0
    for g, (n, limit, keys) in zip(groups, wl.expected_lists(res, labels, b, groups, cfg.topk, False)):
        if n == cfg.topk and [k & 0xFFFFFF for k in keys] == rare[:cfg.topk].tolist():
            got, rounds = wl.emulated_walk(res, labels, req[g], int(b.group_need[g]), cfg.topk, 2, HDR["WK_MULTI"],
                                           HDR["WK_MULTI_AFTER"])
            k = scan_emulator.keys(res, labels, req[g], int(b.group_need[g]), 0)
            collected = int((k[:rounds * HDR["WK_ROUND"]] != scan_emulator.NO_KEY).sum())
            long_walks += rounds * HDR["WK_ROUND"] > rare[cfg.topk] and collected > room
    assert long_walks >= 5, long_walks      # the K smallest keys are the first K rare nodes, found past the compaction


def test_threshold_nodes_sit_on_both_sides_of_every_line_of_node_prep():
    for n in (64, 1023):
        inv, tags = wl.threshold_nodes(n)
        cls, S = wl.node_class(inv.residual())
        names = {0: "never", 1: "walk", 2: "slow"}
        seen = {}
        for i, t in enumerate(tags):
            if t is None:
                assert cls[i] == 1, i
            else:
                assert names[int(cls[i])] == t[1], (i, t, inv.residual()[:, i])
                seen.setdefault(t[0], []).append(i)
        assert set(seen) == {"S=SMAX-1", "S=SMAX", "r0=SMAX", "r0=SMAX+1", "r1=(SMAX-2)<<20|odd", "r1=2^60-1",
                             "r1=2^60", "r2=2^20-1", "r2=2^20", "r3=INT64_MAX", "all INT64_MAX", "all 0", "one -1"}
        assert set(cls.tolist()) == {0, 1, 2} and all(len(v) >= 1 for v in seen.values())
        res = inv.residual()
        assert all(int(S[i]) == wl.SMAX - 1 and res[1, i] & 1 and res[3, i] & 1 for i in seen["S=SMAX-1"])
        assert all(int(S[i]) == wl.SMAX - 2 for i in seen["r1=(SMAX-2)<<20|odd"])
        assert all(int(res[3, i]) >> 24 == (1 << 39) - 1 for i in seen["r3=INT64_MAX"])
        assert sorted(int(res[:, i].argmin()) for i in seen["one -1"]) == [0, 1, 2, 3]
        assert len({(int(res[1, i]) & wl.LO1, int(res[3, i]) & wl.LO3) for i in seen["S=SMAX"]}) == len(seen["S=SMAX"])


def test_threshold_keys_two_restatements_agree_and_the_node_only_form_is_exact():
    """scan_emulator.keys against oracle.key on every (node, request) pair of the thresholds set, before either is
    the reference; and for every walkable node and fitting request K(n) - ((s(q) + borrows) << 24) is that key."""
    import oracle
    inv, _ = wl.threshold_nodes(1023)
    res, labels = inv.residual(), inv.labels
    cls, S = wl.node_class(res)
    batches = (wl.threshold_batch(), wl.threshold_batch(1))
    fast = 0
    for b in batches:
        for q, need in zip(synth.scan_requests(b), b.group_need):
            k = scan_emulator.keys(res, labels, q, int(need), 0)
            q = [int(v) for v in q]
            sq = q[0] + (q[1] >> 20) + (q[2] << 20) + (q[3] >> 24)
            for n in range(inv.n):
                assert int(k[n]) == oracle.key(res[:, n], int(labels[n]), q, int(need), n), (n, q)
                if cls[n] == 1 and int(k[n]) != wl.NO_KEY:
                    bor = ((int(res[1, n]) & wl.LO1) < (q[1] & wl.LO1)) + ((int(res[3, n]) & wl.LO3) < (q[3] & wl.LO3))
                    assert ((int(S[n]) << 24) | n) - ((sq + bor) << 24) == int(k[n]), (n, q, bor)
                    fast += 1
    assert fast >= 5000, fast


def test_threshold_scripts_yield_lists_of_every_kind():
    kinds = dict(full=0, short=0, empty=0, overlay_only=0, score0=0)
    for cfg in wl.EDGE_CONFIGS:
        if cfg.kind != "thresholds":
            continue
        for res, labels, b, groups in states(cfg):
            req = synth.scan_requests(b)
            assert wl.slow_nodes(res).any()
            for g, (n, limit, keys) in zip(groups, wl.expected_lists(res, labels, b, groups, cfg.topk, False)):
                q = [int(v) for v in req[g]]
                sq = q[0] + (q[1] >> 20) + (q[2] << 20) + (q[3] >> 24)
                no_walk = q[0] > wl.SMAX or q[2] >= 1 << 20 or sq >= wl.SMAX
                kinds["full"] += n == cfg.topk and limit != wl.NO_KEY
                kinds["short"] += 0 < n < cfg.topk and limit == wl.NO_KEY
                kinds["empty"] += n == 0
                kinds["overlay_only"] += no_walk and n > 0
                kinds["score0"] += n > 0 and keys[0] >> 24 == 0
    print(kinds)
    assert min(kinds.values()) >= 5, kinds
    for scan in (False, True):
        t = wl.edge_totals(scan)
        print("edge", "scan" if scan else "walk", t)
        assert t.lists >= 400 and t.full >= 100 and t.short >= 50 and t.empty >= 20 and t.overlay >= 80, t
