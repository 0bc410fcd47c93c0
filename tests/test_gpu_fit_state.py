"""The staged fit-mask state across inventory changes, on every fit path, bit-exact against the C
oracle on a host model of the inventory (inventory_model.Model).

One context per path is walked through what a Node informer and a scheduler do to it: a one-shot
mask, the staged form, a greedy placement, a node update batch with removals, a reset, smaller and
larger batches on the warm (grow-only) buffers, and a smaller and a larger inventory.  After every
step the counts, the whole mask and a set of row windows that start and end inside the 16-row tile
bands and the 64-job bands are compared with the oracle, and the path's own stats counter must have
moved by exactly one (a silent fallback to another kernel cannot pass).

pe_load_nodes invalidates the staged batch (include/placement.h): the staged calls are PE_ESTATE
until the next upload, which is all the shrink and grow steps observe of it.

Sizes: 8192 + 777 nodes are two 8192-node blocks with a partial last one, 141 mask words (the last
tile column partial) and a partial last 512-node segment; 130 jobs are no multiple of 16 or 64 and
make three 64-job bands."""
import numpy as np
import pytest

from inventory_model import Model, make_deltas, mask_bits, removed_slots, row_windows
from placement import Engine, PlacementError, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)      # PE_NEED_ISLAND
B17, B30 = np.uint32(1 << 17), np.uint32(1 << 30)
GiB = 1 << 30
N1, N2, N3 = 8192 + 777, 777, 20001
J1, J2, J3 = 130, 17, 321
RUNS = ("fit_runs_planes", "fit_runs_coded", "fit_runs_i32", "fit_runs_i64", "fit_runs_lds")

# fit_path_mask, the counter of the path, further counters that must move by (counter, delta), the
# mask layout, the batch shape, and whether the label needs must form an inclusion chain (the coded
# kernels take nothing else)
PATHS = {
    "planes": (0, "fit_runs_planes", {"fit_runs_sets": 0}, 3, "cfg5", False),
    "planes_blocks": (16 | 32, "fit_runs_planes", {"fit_runs_sets": 0}, 2, "cfg5", False),
    "plane_sets": (16, "fit_runs_planes", {"fit_runs_sets": 1}, 3, "many", False),
    "lds": (64, "fit_runs_lds", {}, 3, "many", False),
    "therm": (5, "fit_runs_coded", {"fit_runs_therm": 1}, 1, "cfg5", True),
    "swar": (13, "fit_runs_coded", {"fit_runs_therm": 0}, 1, "cfg5", True),
    "i32": (3, "fit_runs_i32", {}, 0, "cfg5", False),
    "i64": (1, "fit_runs_i64", {}, 0, "cfg5", False),
}


def make_batch(path, J, seed):
    """cfg5 requests (or the 40-cpu-value batch no single plane set holds), job 0 asking for nothing,
    and label needs beyond bit 0: about a quarter of the jobs need an island, a few bit 17, one bits
    17 and 30 -- four distinct needs besides 0.  For the coded paths they form the chain
    0 < gpu < gpu|island < ..|17 < ..|30; elsewhere {0, gpu, island, 17, 17|30}, which is none."""
    shape, chain = PATHS[path][4], PATHS[path][5]
    req, need = synth.make_fit_jobs(J, seed)         # need: bit 0 where a GPU is requested
    j = np.arange(J)
    if shape == "many":
        req[:, 0] = 500 + (j % 40) * 7
        if J < 40:   # fewer than 40 jobs: memory distinct per job too, so the pairs still pass 32
            req[:, 1] = (1 + j) * GiB
    if chain:
        isl = (need == 1) & (j % 2 == 0)
        need[isl] |= ISLAND
        b17 = np.flatnonzero(isl & (j % 8 == 0) & (j > 0))
        need[b17] |= B17
        need[b17[:1]] |= B30
    else:
        need[j % 4 == 1] = ISLAND
        need[j % 16 == 3] = B17
        need[min(7, J - 1)] = B17 | B30
    req[0], need[0] = 0, 0
    assert len(np.unique(need[need != 0])) <= 4
    return req, need


def make_inventory(N, seed):
    inv = synth.make_inventory(N, seed, 0.4)
    inv.cap[1, ::7] = 1 << 50                                  # past the int32 saturation point
    inv.used[0, 3::11] = inv.cap[0, 3::11] + 1000              # negative residuals
    inv.labels[::5] |= B17
    inv.labels[::7] |= B30
    return inv


class Ctx:
    """An engine on one path and the model of its shard; every fit run is counted."""

    def __init__(self, path, rank=0, world=1):
        self.path = path
        self.bits, self.stat, self.extra, self.layout = PATHS[path][:4]
        self.e = Engine(0, fit_path_mask=self.bits, rank=rank, world_size=world,
                        exchange=(lambda b: b * world) if world > 1 else None)
        self.m = None

    def load(self, inv, model=None):
        self.e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
        b, en = self.e.shard_range()
        self.m = (model or Model.of(inv)).shard(b, en)
        self.Ns = en - b

    def counted(self, fn, *args):
        """fn(*args) must be one run of this path's kernel -- or of none on an empty shard, where
        there is nothing to launch."""
        s0 = self.e.stats()
        out = fn(*args)
        s1 = self.e.stats()
        d = {k: s1[k] - s0[k] for k in s1}
        if self.Ns == 0:
            assert all(d[k] == 0 for k in RUNS + ("fit_runs_sets", "fit_runs_therm")), (self.path, d)
            return out
        assert d[self.stat] == 1, (self.path, d)
        assert sum(d[k] for k in RUNS) == 1, (self.path, d)
        for k, v in self.extra.items():
            assert d[k] == v, (self.path, k, d)
        assert self.e.fit_mask_layout() == self.layout
        return out

    def uncounted(self, fn, *args):
        s0 = self.e.stats()
        out = fn(*args)
        s1 = self.e.stats()
        assert all(s1[k] == s0[k] for k in RUNS), (self.path, s0, s1)
        return out

    def one_shot(self, req, need):
        return self.check(req, need, self.counted(self.e.fit_mask, req, need))

    def upload(self, req, need):
        self.uncounted(self.e.jobs_upload, req, need)

    def rerun(self, req, need):
        self.counted(self.e.fit_mask_run)
        return self.check(req, need, self.e.fit_counts())

    def check(self, req, need, counts):
        """counts, the whole mask and every row window against the oracle on the model."""
        J = len(req)
        o_mask, o_counts = self.m.fit(req, need)
        assert counts.shape == (J,)
        np.testing.assert_array_equal(counts, o_counts, err_msg=f"{self.path}: counts")
        np.testing.assert_array_equal(self.e.fit_counts(), o_counts, err_msg=f"{self.path}: fit_counts")
        W = (self.Ns + 63) // 64
        full = self.uncounted(self.e.fit_mask_rows, 0, J)
        assert full.shape == (J, W)
        np.testing.assert_array_equal(full, o_mask, err_msg=f"{self.path}: mask")
        for r0, n in row_windows(J):
            got = self.e.fit_mask_rows(r0, n)
            assert got.shape == (n, W)
            np.testing.assert_array_equal(got, o_mask[r0:r0 + n], err_msg=f"{self.path}: rows {r0}+{n}")
        return o_mask, o_counts

    def staged_calls_need_an_upload(self):
        s0 = self.e.stats()
        for call in (self.e.fit_mask_run, self.e.fit_counts, lambda: self.e.fit_mask_rows(0, 1)):
            with pytest.raises(PlacementError, match="PE_ESTATE") as ei:
                call()
            assert "pe_jobs_upload first" in str(ei.value)
        s1 = self.e.stats()
        assert all(s1[k] == s0[k] for k in RUNS), (self.path, s0, s1)      # raised before any launch

    def capacity_nodes_equal(self, req, need, counts):
        # a job fits a node exactly when the node holds at least one pod of its shape
        np.testing.assert_array_equal(self.uncounted(self.e.gang_capacity, req, need)[2], counts)


@pytest.mark.parametrize("path", list(PATHS))
def test_sequence(path):
    c = Ctx(path)
    e = c.e
    req, need = make_batch(path, J1, 11)
    # 1. one-shot
    c.load(make_inventory(N1, 5))
    _, cnt1 = c.one_shot(req, need)
    assert cnt1[(need & ISLAND) != 0].sum() > 0 and 0 < cnt1.sum() < N1 * J1
    # 2. staged, and the row-range check
    c.upload(req, need)
    _, cnt2 = c.rerun(req, need)
    np.testing.assert_array_equal(cnt2, cnt1)
    for r0, n in [(-1, 1), (J1, 1), (0, J1 + 1)]:
        with pytest.raises(PlacementError, match="PE_EINVAL"):
            e.fit_mask_rows(r0, n)
    np.testing.assert_array_equal(e.fit_mask_rows(J1 - 3, 3), c.m.fit(req, need)[0][J1 - 3:])
    # 3. after a placement: the same upload, the new residuals
    batch = synth.make_jobs(150, 13, "mixed")
    pods, st = c.uncounted(e.place_batch, batch)
    w_pods, w_st, w_after = c.m.place(batch)
    np.testing.assert_array_equal(pods, w_pods)
    np.testing.assert_array_equal(st, w_st)
    np.testing.assert_array_equal(e.read_residuals(), w_after)
    mask3, cnt3 = c.rerun(req, need)
    assert (cnt3 <= cnt2).all() and (cnt3 < cnt2).any()
    c.capacity_nodes_equal(req, need, cnt3)
    # 4. after node updates with removals
    deltas = make_deltas(N1, 500, 17)
    gone = removed_slots(deltas)
    c.uncounted(e.update_nodes, *deltas)
    c.m.update(deltas)
    np.testing.assert_array_equal(e.read_residuals(), c.m.res)
    mask4, cnt4 = c.rerun(req, need)
    full = e.fit_mask_rows(0, J1)
    was = mask_bits(mask3, gone)
    assert len(gone) and was.any() and was[0].any()      # some removed slot fitted before, job 0 too
    assert not mask_bits(full, gone).any()               # no row fits a removed slot, the all-zero request neither
    c.capacity_nodes_equal(req, need, cnt4)
    # 5. after a reset: the load-time inventory with step 4's updates, not step 3's placements
    c.uncounted(e.reset_residuals)
    c.m.reset()
    np.testing.assert_array_equal(e.read_residuals(), c.m.res)
    _, cnt5 = c.rerun(req, need)
    assert (cnt5 != cnt4).any()
    # 6. a smaller, then a larger batch on the warm buffers
    req2, need2 = make_batch(path, J2, 19)
    c.upload(req2, need2)
    c.rerun(req2, need2)
    assert e.fit_counts().shape == (J2,)
    c.one_shot(*make_batch(path, J3, 23))
    # 7. a smaller inventory: the staged batch is gone
    c.load(make_inventory(N2, 29))
    c.staged_calls_need_an_upload()
    c.one_shot(req, need)
    assert not (e.fit_mask_rows(0, J1)[:, -1] >> np.uint64(N2 % 64)).any()     # nothing at or past node 777
    # 8. a larger one
    c.load(make_inventory(N3, 31))
    c.staged_calls_need_an_upload()
    c.one_shot(req, need)
    assert not (e.fit_mask_rows(0, J1)[:, -1] >> np.uint64(N3 % 64)).any()
    e.close()


@pytest.mark.parametrize("path", ["planes", "lds", "i32"])
def test_sequence_sharded(path):
    """Two shard contexts (host exchange): the one-shot mask and the run after an update batch that
    every rank receives whole; each shard against its slice of the model, the counts summed over the
    shards against the unsharded oracle."""
    req, need = make_batch(path, J1, 41)
    inv = make_inventory(N1, 43)
    whole = Model.of(inv)
    deltas = make_deltas(N1, 500, 47)
    _, want1 = whole.fit(req, need)
    whole.update(deltas)
    _, want4 = whole.fit(req, need)
    gone = removed_slots(deltas)
    tot1, tot4 = np.zeros(J1, np.int64), np.zeros(J1, np.int64)
    for rank in range(2):
        c = Ctx(path, rank, 2)
        c.load(inv)
        b, en = c.e.shard_range()
        assert (b, en) == (N1 * rank // 2, N1 * (rank + 1) // 2)
        tot1 += c.one_shot(req, need)[1]
        c.uncounted(c.e.update_nodes, *deltas)
        c.m = whole.shard(b, en)
        np.testing.assert_array_equal(c.e.read_residuals(), c.m.res)
        o_mask, o_cnt = c.rerun(req, need)
        mine = gone[(gone >= b) & (gone < en)] - b
        assert len(mine) and not mask_bits(c.e.fit_mask_rows(0, J1), mine).any()
        tot4 += o_cnt
        c.e.close()
    np.testing.assert_array_equal(tot1, want1)
    np.testing.assert_array_equal(tot4, want4)
    assert (want1 != want4).any()


@pytest.mark.parametrize("path", list(PATHS))
def test_empty_shard(path):
    """Two nodes over four ranks: ranks 0 and 2 hold nothing (all-zero counts, a [J][0] mask, PE_OK
    from the staged calls, zero capacity, no kernel run); ranks 1 and 3 hold one node each and answer
    as the oracle does."""
    inv = make_inventory(2, 53)
    whole = Model.of(inv)
    req, need = make_batch(path, J2, 59)
    _, want = whole.fit(req, need)
    total = np.zeros(J2, np.int64)
    empty = 0
    for rank in range(4):
        c = Ctx(path, rank, 4)
        c.load(inv)
        b, en = c.e.shard_range()
        assert (b, en) == (2 * rank // 4, 2 * (rank + 1) // 4)
        _, cnt = c.one_shot(req, need)
        c.upload(req, need)
        c.rerun(req, need)
        cap = c.uncounted(c.e.gang_capacity, req, need)
        np.testing.assert_array_equal(cap[2], cnt)
        if en == b:
            empty += 1
            np.testing.assert_array_equal(c.e.fit_mask(req, need), np.zeros(J2, np.int64))
            assert c.e.fit_mask_rows(0, J2).shape == (J2, 0)
            for a in cap:
                assert not a.any()
        total += cnt
        c.e.close()
    assert empty == 2
    np.testing.assert_array_equal(total, want)
