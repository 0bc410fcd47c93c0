"""The candidate lists of the real engine's windows, list by list.  One context per configuration is walked through
window_lists.script(): small pe_place_greedy calls of at most one window each, most without a reset in between, with
pe_update_nodes and a reset on the way.  Before every call the residuals are read back; PE_DUMP_WINDOWS records the
call's first window; every list of it must be TIGHT against scan_emulator.keys over those residuals: n, every key
and the limit exact (window_lists.expected_lists; the contract is stated in cand_lists.py).  The end-to-end suites
compare placements, which a list that is merely sound -- too short, its limit too low -- never changes."""
import os
import time

import numpy as np
import pytest

import window_lists as wl
from inventory_model import Model
from placement import Engine

pytestmark = pytest.mark.gpu


def walk_config(mode, cfg, tmp_path, monkeypatch, tally):
    kwargs, env = wl.MODES[mode]
    scan = mode in wl.SCAN_MODES
    dump = str(tmp_path / "window.bin")
    eng = Engine(0, topk=cfg.topk, **kwargs)
    try:
        m = None
        for i, st in enumerate(wl.script(cfg)):
            if st.op == "load":
                inv = st.arg
                eng.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
                m = Model.of(inv)
            elif st.op == "update":
                eng.update_nodes(*st.arg)
                m.update(st.arg)
            elif st.op == "reset":
                eng.reset_residuals()
                m.reset()
            else:
                res = eng.read_residuals()
                assert np.array_equal(res, m.res), (mode, cfg, i)
                s0 = eng.stats()
                if os.path.exists(dump):
                    os.remove(dump)
                with monkeypatch.context() as mp:
                    for k, v in env.items():
                        mp.setenv(k, v)
                    mp.setenv("PE_DUMP_WINDOWS", dump)
                    mp.setenv("PE_DUMP_MAX_WINDOWS", "1")
                    eng.place_batch(st.arg)
                s1 = eng.stats()
                m.place(st.arg)
                stride, groups, lists, _ = wl.read_dump(dump)
                assert stride >= cfg.topk and groups == wl.first_window(st.arg).tolist()
                want = wl.expected_lists(res, m.labels, st.arg, groups, cfg.topk, scan)
                assert len({flags for _, flags, _, _ in lists}) == 1, "one window, one generation"
                for g, (n, flags, limit, keys), (wn, wlimit, wkeys) in zip(groups, lists, want):
                    where = (mode, cfg, "call %d group %d" % (i, g))
                    assert (n, limit) == (wn, wlimit), (where, "n, limit", n, hex(limit), wn, hex(wlimit))
                    assert keys == wkeys, (where, "keys differ first at",
                                           next(j for j in range(n) if keys[j] != wkeys[j]))
                    tally["full"] += n == cfg.topk and limit != wl.NO_KEY
                    tally["short"] += 0 < n < cfg.topk and (scan or limit == wl.NO_KEY)
                    tally["empty"] += n == 0
                tally["lists"] += len(groups)
                one = s1["windows"] - s0["windows"] == 1
                if not scan and one and s1["walk_overlay"] > s0["walk_overlay"]:
                    tally["overlay"] += len(groups)     # the window's groups evaluated overlay entries
                if not scan and one and s1["resorts"] > s0["resorts"]:
                    tally["rebuilt"] += len(groups)     # the index was rebuilt or taken over right before the window
    finally:
        eng.close()


@pytest.mark.parametrize("mode", sorted(wl.MODES))
def test_first_window_lists_are_tight(mode, tmp_path, monkeypatch):
    tally = dict(lists=0, full=0, short=0, empty=0, overlay=0, rebuilt=0)
    for cfg in wl.CONFIGS:
        walk_config(mode, cfg, tmp_path, monkeypatch, tally)
    print(mode, tally)
    scan = mode in wl.SCAN_MODES
    need = wl.totals(scan)      # (test_cand_lists_cpu.py: the model alone yields enough lists of every kind)
    assert (tally["lists"], tally["full"], tally["short"], tally["empty"]) == need[:4], (tally, need)
    if not scan:
        # a call that rescans runs more than one window and its counters cannot be told apart: at least half of
        # the calls the model names must have been counted
        assert tally["overlay"] >= need.overlay // 2 and tally["rebuilt"] >= need.lists // 2, (tally, need)


@pytest.mark.parametrize("mode", sorted(wl.MODES))
def test_first_window_lists_are_tight_at_key_edges(mode, tmp_path, monkeypatch):
    """EDGE_CONFIGS: low bits in residuals and requests, so that keys borrow and K(n) order is not key order (the
    walk's stop bound, its start round, fast_key's carry into the high word, the low parts apply and the scatter
    keep), and nodes and requests on node_prep's and s(q)'s saturation lines.  test_window_lists_cpu.py shows on
    the model alone that a walk with less slack, and nothing in CONFIGS, fails exactly here."""
    tally = dict(lists=0, full=0, short=0, empty=0, overlay=0, rebuilt=0)
    t0 = time.perf_counter()
    for cfg in wl.EDGE_CONFIGS:
        walk_config(mode, cfg, tmp_path, monkeypatch, tally)
    print(mode, tally, "%.2f s" % (time.perf_counter() - t0))
    scan = mode in wl.SCAN_MODES
    need = wl.edge_totals(scan)
    assert (tally["lists"], tally["full"], tally["short"], tally["empty"]) == need[:4], (tally, need)
    if not scan:
        assert tally["overlay"] >= need.overlay // 2 and tally["rebuilt"] >= need.lists // 2, (tally, need)
