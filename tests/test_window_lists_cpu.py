"""window_lists.py on the host model alone: the script of test_gpu_window_lists.py yields lists of every kind -- full
with a real limit, short with the bound as limit, empty, taken with saturating nodes in the overlay -- at every topk,
node count and inventory kind, and its calls are one window each; scan_bound against a plain loop; read_dump on a
file written here in the engine's layout."""
import struct

import numpy as np

import scan_emulator
import window_lists as wl
from placement import synth


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
