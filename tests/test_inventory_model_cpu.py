"""The inventory model the stateful fit-mask suite compares the engine with (inventory_model.py):
the properties of it that the GPU tests lean on, checked without a GPU."""
import numpy as np

from inventory_model import NEVER, Model, mask_bits, row_windows
from placement import PE_NODE_REMOVE, PE_NODE_SET, synth


def one_delta(slot, op, res4=(0, 0, 0, 0), labels=0, island=-1):
    cap = np.array([res4], dtype=np.int64)
    return (np.array([slot]), np.array([op], np.uint8), cap, np.zeros_like(cap), np.array([labels], np.uint32),
            np.array([island], np.int32))


def test_remove_clears_the_column_for_every_job():
    m = Model.of(synth.make_inventory(200, 3, 0.4))
    req, need = synth.make_fit_jobs(50, 5)
    req[0], need[0] = 0, 0                                   # the all-zero request fits any live node
    slot = int(np.flatnonzero((m.res >= 0).all(axis=0))[0])
    before, _ = m.fit(req, need)
    assert mask_bits(before, [slot])[0, 0] == 1
    m.update(one_delta(slot, PE_NODE_REMOVE))
    after, counts = m.fit(req, need)
    assert not mask_bits(after, [slot]).any()
    assert (m.res[:, slot] == NEVER).all() and (m.res0[:, slot] == NEVER).all()
    assert counts[0] == np.unpackbits(before[0].view(np.uint8)).sum() - 1      # only that node left the row


def test_set_then_reset_returns_the_set_values():
    inv = synth.make_inventory(100, 7, 0.4)
    m = Model.of(inv)
    m.place(synth.make_jobs(20, 9, "mixed"))
    assert (m.res != m.res0).any()
    m.update(one_delta(11, PE_NODE_SET, (7, 8, 9, 10), labels=1 << 17, island=4))
    m.res[:, 11] -= 1                                        # (as a placement would)
    m.reset()
    np.testing.assert_array_equal(m.res[:, 11], [7, 8, 9, 10])
    assert m.labels[11] == (1 << 17) | (1 << 31)             # bit 31 from the island, as the engine keeps it
    keep = np.arange(100) != 11
    np.testing.assert_array_equal(m.res[:, keep], inv.residual()[:, keep])


def test_row_windows_stay_inside_and_cut_the_bands():
    for J in (1, 16, 17, 64, 65, 130):
        ws = row_windows(J)
        assert (J, 0) in ws and (0, 1) in ws and len(set(ws)) == len(ws)
        assert all(0 <= r0 and 0 <= n and r0 + n <= J for r0, n in ws)
        if J >= 65:
            for band in (16, 64):   # a window that starts and ends strictly inside a band
                assert any(n > 0 and r0 % band and (r0 + n) % band for r0, n in ws), (J, band)
            assert any(r0 // 16 != (r0 + n - 1) // 16 and r0 % 16 for r0, n in ws if n)   # and crosses an edge
            assert any(r0 // 64 != (r0 + n - 1) // 64 and r0 % 64 for r0, n in ws if n)
