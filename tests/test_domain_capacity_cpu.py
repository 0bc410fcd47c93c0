"""The per-domain capacity checker (tests/domain_capacity.py) against hand-worked cells, the whole-shard
checker and the C oracle's greedy placement; the selection rule; the ABI surface of
pe_gang_capacity_domains that needs no GPU."""
import numpy as np
import pytest

import domain_capacity as DC
import gang_capacity as G
import oracle
from placement import _abi, select_domain, synth
from test_go_binding import HIP_GO, go_calls, header_arity


def test_special_cells_by_hand():
    cap, used, labels, island, D = DC.special_domains()
    res, lab = cap - used, synth.island_labels(labels, island)
    req = [c[0] for c in G.SPECIAL_CASES]
    need = [c[1] for c in G.SPECIAL_CASES]
    slots, nodes = DC.tables(res, lab, island, req, need, D)
    assert slots.shape == nodes.shape == (len(req), D)
    for j, (want_slots, want_nodes) in enumerate(DC.special_tables()):
        assert [int(x) for x in slots[j]] == want_slots, (j, req[j])
        assert [int(x) for x in nodes[j]] == want_nodes, (j, req[j])
    # a few cells spelled out: [1, 1, 1, 1] -> domain 2 = node 0 (4) + node 1 (CAP_MAX); all-zero request ->
    # domain 2 = 2 x CAP_MAX, domain 0 = node 2 = CAP_MAX, node 4 (CAP_MAX, no domain) and node 3 (domain 5) nowhere
    assert [int(x) for x in slots[3]] == [0, 0, 4 + G.CAP_MAX, 0] and [int(x) for x in nodes[3]] == [0, 0, 2, 0]
    assert [int(x) for x in slots[0]] == [G.CAP_MAX, 0, 2 * G.CAP_MAX, 0] and [int(x) for x in nodes[0]] == [1, 0, 2, 0]
    assert [int(x) for x in slots[4]] == [1, 0, 1 + G.CAP_MAX, 0]       # [7, 0, 3, 9]: node 2 holds exactly one


@pytest.mark.parametrize("name", ["racks32", "interleaved", "own", "one"])
def test_identity_with_the_whole_shard(name):
    """Every id below n_domains: the domains add up to gang_capacity's answer for need | ISLAND."""
    inv = synth.make_inventory(700, 7)
    island, D = DC.layout(name, 700)
    island = np.where(np.arange(700) % 5 == 0, -1, island).astype(np.int32)   # some nodes of no domain
    cap, used, lab, island = DC.with_islands(inv, island)
    req, need = synth.make_fit_jobs(60, 7)
    slots, nodes = DC.tables(cap - used, lab, island, req, need, D)
    w_slots, _, w_nodes = G.capacity(cap - used, lab, req, (need | np.uint32(G.ISLAND)).astype(np.uint32))
    np.testing.assert_array_equal(slots.sum(axis=1), w_slots)
    np.testing.assert_array_equal(nodes.sum(axis=1), w_nodes)
    assert w_slots.any() and (w_slots < G.capacity(cap - used, lab, req, need)[0]).any()


def placed(res, labels, count, req, need):
    _, st, _ = oracle.place_greedy(res, labels, *G.one_group_batch(count, req, need))
    return int(st[0]) == 0


@pytest.mark.parametrize("req,need", G.greedy_shapes())
def test_oracle_greedy_fills_a_domain_exactly(req, need):
    """On the nodes of one domain alone the oracle's greedy places a one-group gang of exactly dom_slots
    pods and fails at dom_slots + 1."""
    inv = G.greedy_inventory()
    island = (np.arange(200) % 8).astype(np.int32)
    cap, used, lab, island = DC.with_islands(inv, island)
    res = cap - used
    slots, nodes = DC.tables(res, lab, island, [req], [need], 8)
    assert (slots[0] >= 2).sum() >= 4 and (nodes[0] <= 25).all()
    for k in range(8):
        on = island == k
        s = int(slots[0, k])
        r, l = np.ascontiguousarray(res[:, on]), np.ascontiguousarray(lab[on])
        if s >= 1:
            assert placed(r, l, s, req, need), (k, s)
        assert not placed(r, l, s + 1, req, need), (k, s)


def test_selection_rule():
    table = np.array([[5, 9, 5, 0, 12],       # ties
                      [5, 9, 5, 0, 12],
                      [5, 9, 5, 0, 12],
                      [5, 9, 5, 0, 12],
                      [0, 0, 0, 0, 0],
                      [2**55, 7, 2**55, 7, 8]], dtype=np.int64)
    count = np.array([5, 6, 13, 1, 1, 8], dtype=np.int32)
    dom, slots, feas = DC.select(table, count)
    assert dom.tolist() == [0, 1, -1, 0, -1, 4]          # count == a domain's slots; tie -> smallest id; none
    assert slots.tolist() == [5, 9, 0, 5, 0, 8]
    assert feas.tolist() == [4, 2, 0, 4, 0, 3]
    assert DC.select_row([3, 3, 3], 3) == (0, 3, 3) and DC.select_row([3, 3, 3], 4) == (-1, 0, 0)
    # the package's host helper (tables added over shards) follows the same rule
    for got, want in zip(select_domain(table, count), (dom, slots, feas)):
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    rng = np.random.default_rng(3)
    t = rng.integers(0, 6, (200, 9)).astype(np.int64)
    c = rng.integers(1, 7, 200).astype(np.int32)
    for got, want in zip(select_domain(t, c), DC.select(t, c)):
        np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        select_domain(t, np.zeros(200, dtype=np.int32))


def test_bindings():
    """The header declares pe_gang_capacity_domains with 11 arguments; _abi.py and hip.go bind it so."""
    assert header_arity()["pe_gang_capacity_domains"] == 11
    res, args = _abi.SIGNATURES["pe_gang_capacity_domains"]
    assert len(args) == 11 and args[5] is _abi.i32
    assert go_calls(HIP_GO)["pe_gang_capacity_domains"] == {11}
    assert "func (e *Engine) GangCapacityDomains(" in open(HIP_GO).read()
    assert _abi.PE_MAX_DOMAINS == 65536
    header = open(_abi.HEADER).read()
    assert "#define PE_MAX_DOMAINS 65536" in header and "#define PE_ABI_VERSION 7" in header
    lib = _abi.load()
    assert lib.pe_gang_capacity_domains(None, 0, None, None, None, 1, None, None, None, None, None) == _abi.PE_EINVAL
