"""The gang-capacity checker (tests/gang_capacity.py) against code it shares no line with: the C oracle's
fit mask and greedy placement, and hand-worked cells.  Plus the ABI surface of pe_gang_capacity that
needs no GPU."""
import numpy as np
import pytest

import gang_capacity as G
import oracle
from placement import _abi, synth


def test_special_cells_by_hand():
    cap, used, labels, island = G.special_inventory()
    res, lab = cap - used, synth.island_labels(labels, island)
    for q, nd, want in G.SPECIAL_CASES:
        got = G.capacity_matrix(res, lab, [q], [nd])[0]
        assert list(got) == want, (q, nd)
        assert [G.cap_cell(res[:, n], lab[n], q, nd) for n in range(res.shape[1])] == want, (q, nd)
        slots, max_node, nodes = G.capacity(res, lab, [q], [nd])
        assert (slots[0], max_node[0], nodes[0]) == (sum(want), max(want), sum(1 for w in want if w >= 1))


def test_fit_mask_agreement():
    inv = synth.make_inventory(3000, 7)
    req, need = synth.make_fit_jobs(300, 7)
    m = G.capacity_matrix(inv.residual(), inv.labels, req, need)
    slots, max_node, nodes = G.capacity(inv.residual(), inv.labels, req, need)
    o_mask, o_counts = oracle.fit_mask(inv.residual(), inv.labels, req, need)
    np.testing.assert_array_equal(nodes, o_counts)
    bits = np.unpackbits(o_mask.view(np.uint8), axis=1, bitorder="little")[:, :3000].astype(bool)
    np.testing.assert_array_equal(np.asarray(m >= 1, dtype=bool), bits)
    assert (slots >= nodes).all() and (max_node <= slots).all() and nodes.max() > 0


def placed(inv, count, req, need):
    _, st, _ = oracle.place_greedy(inv.residual(), inv.labels, *G.one_group_batch(count, req, need))
    return int(st[0]) == 0


@pytest.mark.parametrize("req,need", G.greedy_shapes())
def test_greedy_agreement_ordinary_group(req, need):
    """A one-group gang is placeable exactly up to `slots` pods."""
    inv = G.greedy_inventory()
    slots, _, _ = G.capacity(inv.residual(), inv.labels, [req], [need])
    s = int(slots[0])
    assert 2 <= s <= 520
    assert placed(inv, s - 1, req, need) and placed(inv, s, req, need) and not placed(inv, s + 1, req, need)


@pytest.mark.parametrize("req,need", G.greedy_island_shapes())
def test_greedy_agreement_island_group(req, need):
    """An island gang (all pods on one node) is placeable exactly up to `max_node` pods."""
    inv = G.greedy_inventory()
    slots, max_node, _ = G.capacity(inv.residual(), inv.labels, [req], [need])
    m = int(max_node[0])
    assert 2 <= m < int(slots[0])
    assert placed(inv, m - 1, req, need) and placed(inv, m, req, need) and not placed(inv, m + 1, req, need)


def test_edge_inputs_cover_the_arithmetic():
    """The shared edge inputs reach saturation, exact multiples and every bit length."""
    cap, used, labels, island = G.edge_inventory()
    assert (used == 0).all() and cap.min() == 0 and cap.max() == G.I63
    lengths = {int(v).bit_length() for v in cap.reshape(-1)}
    assert lengths == set(range(64))
    req, need = G.edge_shapes()
    assert {int(v) for v in req.reshape(-1)} >= {0, 1, G.I63}
    _, max_node, nodes = G.capacity(cap, synth.island_labels(labels, island), req[:16], need[:16])
    assert (max_node == G.CAP_MAX).any() and (nodes > 0).all()


def test_abi_without_gpu():
    assert len(_abi.SIGNATURES["pe_gang_capacity"][1]) == 7
    assert _abi.PE_CAP_MAX == G.CAP_MAX == 2147483647
    lib = _abi.load()
    assert lib.pe_gang_capacity(None, 0, None, None, None, None, None) == _abi.PE_EINVAL
