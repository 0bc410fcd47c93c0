"""The device-resident fit mask, read where pe_fit_mask's *dev_mask points and compared word for word with the
layouts include/placement.h publishes (mask_layout.py: the header's formulas, no engine code).

Reference: oracle.fit_mask on the shard's residuals and labels, pushed through mask_layout.image -- the whole extent
the layout's formula addresses, bit exact.  Left out of the comparison, by position, is only what the header calls
unspecified: rows J .. 16 * ceil(J / 16) - 1 of PE_MASK_NODE_TILES (the job table is padded with a request that a
node with INT64_MAX everywhere and every label still fits -- the `max` inventories below hold such a node).  Every
other padding position is promised zero and checked as zero.  pe_fit_mask_rows must agree with mask_layout.rows_of
of the raw words in every case.

Every case forces its kernel through pe_config.fit_path_mask (and PE_LDS_W) and asserts the path's stats counter.

A context's fit_path_mask is fixed when it is created, PE_MASK_NODE_BLOCKS needs its bit 5, and with every path
allowed a batch of at most 300 jobs only ever reaches the three row-major kernels (one plane set, LDS digit planes,
plane sets): the LDS path refuses a batch only for more than 64 distinct label needs, and such a batch cannot form
the inclusion chain the coded path needs.  So test_one_context_many_batches walks three contexts: all paths
(fit_path_mask 0: the three PE_MASK_ROWS kernels at their different pitches), all paths with bit 5 (NODE_BLOCKS ->
ROWS -> NODE_TILES) and the coded and compare paths alone (JOB_BITS <-> NODE_TILES)."""
import contextlib
import os

import numpy as np
import pytest

import gang_ledger as GL
import mask_layout as ML
import oracle
from inventory_model import Model, make_deltas, removed_slots
from placement import PE_NODE_REMOVE, Engine, PlacementError, synth

pytestmark = pytest.mark.gpu

ISLAND = np.uint32(1 << 31)      # PE_NEED_ISLAND
B17 = np.uint32(1 << 17)
GiB = 1 << 30
I64MAX = np.iinfo(np.int64).max
NEVER = np.iinfo(np.int64).min
RUNS = ("fit_runs_planes", "fit_runs_coded", "fit_runs_i32", "fit_runs_i64", "fit_runs_lds")

# path: fit_path_mask, its stats counter, further counters that must move by (counter, delta), the layout, the batch
# kind, PE_LDS_W
PATHS = {
    "i64": (1, "fit_runs_i64", {}, ML.NODE_TILES, "cfg5", None),
    "i32": (3, "fit_runs_i32", {}, ML.NODE_TILES, "cfg5", None),
    "swar": (13, "fit_runs_coded", {"fit_runs_therm": 0}, ML.JOB_BITS, "chain", None),
    "therm": (5, "fit_runs_coded", {"fit_runs_therm": 1}, ML.JOB_BITS, "chain", None),
    "planes": (16, "fit_runs_planes", {"fit_runs_sets": 0}, ML.ROWS, "cfg5", None),
    "planes_blocks": (16 | 32, "fit_runs_planes", {"fit_runs_sets": 0}, ML.NODE_BLOCKS, "cfg5", None),
    "plane_sets": (16, "fit_runs_planes", {"fit_runs_sets": 1}, ML.ROWS, "many", None),
    "lds1": (64, "fit_runs_lds", {}, ML.ROWS, "many", 1),
    "lds2": (64, "fit_runs_lds", {}, ML.ROWS, "many", 2),
    "lds4": (64, "fit_runs_lds", {}, ML.ROWS, "many", 4),
}

# (nodes, jobs) on both sides of each path's seams: 16-job and 256-node tiles (grid rows of 256 jobs); 64-job bands
# and the 1024-node stride (500 and 1500 tell it from a rounding to 512); 8192-node blocks; the LDS block 2048 W
TILE_SIZES = [(1, 1), (63, 15), (64, 16), (65, 17), (255, 63), (256, 64), (257, 65), (1023, 130), (1025, 257), (8193, 17)]
BAND_SIZES = [(1, 1), (63, 63), (64, 64), (65, 65), (500, 65), (1023, 130), (1024, 64), (1025, 65), (1500, 130),
              (2049, 257), (8193, 17)]
BLOCK_SIZES = [(1, 1), (65, 17), (257, 65), (8191, 63), (8192, 64), (8193, 65), (16385, 130), (500, 257)]
SIZES = {
    "i64": TILE_SIZES, "i32": TILE_SIZES, "swar": BAND_SIZES, "therm": BAND_SIZES,
    "planes": BLOCK_SIZES, "planes_blocks": BLOCK_SIZES,
    "plane_sets": [(1, 15)] + BLOCK_SIZES[1:],          # (a single job is one plane set)
    "lds1": [(1, 1), (1025, 17), (2048, 16), (2049, 65), (8193, 130)],
    "lds2": [(2049, 15), (4096, 64), (4097, 65), (16385, 257)],
    "lds4": [(65, 1), (8191, 63), (8192, 64), (8193, 65), (16385, 130)],
}
VARIANTS = ("plain", "max", "neg", "removed")
CASES = [(p, N, J, VARIANTS[(i + k) % 4]) for k, p in enumerate(PATHS) for i, (N, J) in enumerate(SIZES[p])]

# the same kernels where the contexts of test_one_context_many_batches_* reach them (the planner's own LDS block size)
MIXED = {
    "lds_any": (0, "fit_runs_lds", {}, ML.ROWS, "many", None),
    "blocks_any": (0, "fit_runs_planes", {"fit_runs_sets": 0}, ML.NODE_BLOCKS, "cfg5", None),
    "tiles_any": (0, "fit_runs_i32", {}, ML.NODE_TILES, "needs70", None),
    "coded_any": (0, "fit_runs_coded", {}, ML.JOB_BITS, "chain", None),
}


def make_batch(kind, J, seed):
    """cfg5 requests; `many`: 40 cpu values (fewer than 40 jobs: cpu, memory and ephemeral storage distinct per job),
    more than any single plane set holds; `needs70`: 70 distinct label needs, more than the LDS path takes.  Jobs 0 and
    J - 1 ask for nothing: a set bit in the first and in the last tile band and job band of every node that fits
    anything.  Needs: `chain` {0, gpu, gpu|island} (all the coded kernels take), else {0, gpu, island, bit 17}."""
    req, need = synth.make_fit_jobs(J, seed)
    j = np.arange(J)
    if kind in ("many", "needs70"):
        req[:, 0] = 500 + (j % 40) * 7
        if J < 40:
            req[:, 1] = (1 + j) * GiB
            req[:, 3] = (1 + j) * 3 * GiB
    if kind == "chain":
        need[(need == 1) & (j % 2 == 0)] |= ISLAND
    elif kind == "needs70":
        need[:] = ((j % 70) << 1).astype(np.uint32)
    else:
        need[j % 4 == 1] = ISLAND
        need[j % 16 == 3] = B17
    req[0], need[0] = 0, 0
    req[J - 1], need[J - 1] = 0, 0
    return req, need


def mostly_ones_batch(J):
    """Rows that are nearly all ones: tiny requests, no needs, three values in all (one plane set)."""
    req = np.zeros((J, 4), dtype=np.int64)
    req[1::3, 0] = 1
    req[2::3, 1] = 1
    return req, np.zeros(J, dtype=np.uint32)


class Shard:
    """The host's view of what a context holds: residuals and labels (bit 31 from the island) of the GLOBAL
    inventory; the oracle answers for a shard's slice of it."""

    def __init__(self, N, seed, variant):
        inv = synth.make_inventory(N, seed, 0.4)
        inv.cap[1, ::7] = 1 << 50                              # past the int32 saturation point
        inv.labels[::5] |= B17
        inv.labels |= (np.arange(N, dtype=np.uint32) % 64) << np.uint32(1)      # every one of needs70's label sets
        self.gone = np.zeros(0, dtype=np.int64)
        if variant == "neg":                                   # over-committed nodes, not the last one
            over = np.arange(3, N - 1, 11)
            inv.used[0, over] = inv.cap[0, over] + 1000
        elif variant == "max":                                 # INT64_MAX everywhere and every label: the last node
            for n in {N // 2, N - 1}:                          # and one in the middle
                inv.cap[:, n], inv.used[:, n] = I64MAX, 0
                inv.labels[n], inv.island[n] = 0x7FFFFFFF, n
        elif variant == "removed":
            self.gone = np.array(sorted({0, N // 3} - {N - 1}), dtype=np.int64)
        self.inv, self.variant = inv, variant
        self.res = inv.residual()
        self.labels = synth.island_labels(inv.labels, inv.island)

    def load(self, e):
        e.load_nodes(self.inv.cap, self.inv.used, self.inv.labels, self.inv.island)
        if len(self.gone):
            e.update_nodes(self.gone, np.full(len(self.gone), PE_NODE_REMOVE, np.uint8))
            self.res[:, self.gone] = NEVER
            self.labels[self.gone] = 0

    def clean(self):
        """No node that nothing fits: the all-zero request's row is then all ones."""
        return self.variant in ("plain", "max") and not len(self.gone)


@contextlib.contextmanager
def lds_w(W):
    old = os.environ.get("PE_LDS_W")
    if W is not None:
        os.environ["PE_LDS_W"] = str(W)
    try:
        yield
    finally:
        if W is not None:
            if old is None:
                os.environ.pop("PE_LDS_W", None)
            else:
                os.environ["PE_LDS_W"] = old


@pytest.fixture(scope="module")
def engines():
    """One context per fit_path_mask for the whole module (the shard tests make their own)."""
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Engine(0, fit_path_mask=bits)
        return made[bits]

    yield get
    for e in made.values():
        e.close()


def counted(e, path, fn, *args):
    """fn(*args) is exactly one run of the path's kernel."""
    _, stat, extra, layout, _, W = PATHS.get(path) or MIXED[path]
    s0 = e.stats()
    with lds_w(W):
        out = fn(*args)
    s1 = e.stats()
    d = {k: s1[k] - s0[k] for k in s1}
    assert d[stat] == 1 and sum(d[k] for k in RUNS) == 1, (path, d)
    for k, v in extra.items():
        assert d[k] == v, (path, k, d)
    assert e.fit_mask_layout() == layout, path
    return out


def expected(e, res, labels, req, need):
    """(oracle rows, oracle counts, layout, S, pitch) of the context's shard."""
    b, en = e.shard_range()
    o_mask, o_counts = oracle.fit_mask(res[:, b:en], labels[b:en], req, need)
    return o_mask, o_counts, e.fit_mask_layout(), en - b, e.fit_mask_row_pitch()


def check_image(e, res, labels, req, need, counts=None, bit_planes=None, ptr=None):
    """The whole extent at the held pointer against the oracle's image; the gather against the raw words."""
    J = len(req)
    o_mask, o_counts, layout, S, pitch = expected(e, res, labels, req, need)
    # what makes the comparison bite, on the oracle's output
    assert (o_mask[:, (S - 1) // 64] >> np.uint64((S - 1) % 64) & np.uint64(1)).any(), "the last node fits no job"
    if J > 64 and layout == ML.JOB_BITS:
        assert o_mask[64:].any()
    if J > 16 and layout == ML.NODE_TILES:
        assert o_mask[16:].any()
    if layout == ML.ROWS:
        ML.check_pitch(S, pitch, bit_planes)
    else:
        assert pitch == 0
    if ptr is not None:
        assert e.mask_ptr == ptr
    n = ML.extent(layout, J, S, pitch)
    got = e.read_mask_words(n)
    want = ML.image(o_mask, layout, J, S, pitch)
    keep = ~ML.unspecified(layout, J, S, pitch)
    bad = np.flatnonzero((got != want) & keep)
    assert not len(bad), (f"layout {layout} J {J} S {S} pitch {pitch}: {len(bad)} words differ, first at {bad[:8].tolist()}: "
                          f"{got[bad[:4]].tolist()} for {want[bad[:4]].tolist()}")
    np.testing.assert_array_equal(ML.rows_of(got, layout, J, S, pitch), o_mask)
    np.testing.assert_array_equal(e.fit_mask_rows(0, J), ML.rows_of(got, layout, J, S, pitch))
    np.testing.assert_array_equal(e.fit_counts() if counts is None else counts, o_counts)
    assert n == e.mask_extent()                          # the binding's bound is the header's extent
    with pytest.raises(PlacementError, match="PE_EINVAL"):
        e.read_mask_words(n + 1)
    return o_mask


def is_planes(path):
    return path.startswith("planes") or path == "plane_sets"


@pytest.mark.parametrize("path,N,J,variant", CASES, ids=[f"{p}-{N}x{J}-{v}" for p, N, J, v in CASES])
def test_image_per_path(engines, path, N, J, variant):
    bits, kind = PATHS[path][0], PATHS[path][4]
    e = engines(bits)
    sh = Shard(N, 7 + N + J, variant)
    sh.load(e)
    req, need = make_batch(kind, J, 11 + J)
    counts = counted(e, path, e.fit_mask, req, need)
    assert e.words_per_row == ML.words_per_row(N)
    o_mask = check_image(e, sh.res, sh.labels, req, need, counts, is_planes(path))
    if sh.clean():       # the all-zero request: all ones up to the last node, nothing after it
        ones = np.full(ML.words_per_row(N), ~np.uint64(0), dtype=np.uint64)
        if N % 64:
            ones[-1] = np.uint64((1 << (N % 64)) - 1)
        np.testing.assert_array_equal(o_mask[0], ones)
        np.testing.assert_array_equal(o_mask[J - 1], ones)
    if variant == "neg" and N > 4:
        assert not (o_mask[0, 0] >> np.uint64(3)) & np.uint64(1)       # node 3 is over-committed
    if variant == "removed" and N > 1:
        assert not (o_mask[:, 0] & np.uint64(1)).any()                 # node 0 is gone


def test_variants_cover_the_inputs():
    """Some case of every layout has over-committed nodes, some INT64_MAX capacities, some a removed slot."""
    for layout in ML.LAYOUTS:
        seen = {v for p, N, J, v in CASES if PATHS[p][3] == layout and N > 4}
        assert seen == set(VARIANTS), (layout, seen)


def test_no_pointer_no_read():
    e = Engine(0, fit_path_mask=1)
    with pytest.raises(PlacementError, match="PE_ESTATE"):
        e.read_mask_words(1)
    sh = Shard(65, 3, "plain")
    sh.load(e)
    req, need = make_batch("cfg5", 17, 5)
    e.fit_mask(req, need)
    assert e.mask_ptr and len(e.read_mask_words(e.mask_extent())) == 2 * 1 * 64
    sh.load(e)                                   # pe_load_nodes ends the pointer's life
    with pytest.raises(PlacementError, match="PE_ESTATE"):
        e.read_mask_words(1)
    e.close()


# ---------------------------------------------------------------- one context, many batches

def step(e, sh, path, req, need):
    counts = counted(e, path, e.fit_mask, req, need)
    check_image(e, sh.res, sh.labels, req, need, counts, is_planes(path))


def test_one_context_many_batches_rows(engines):
    """Every path allowed: a large batch of nearly all-ones rows, a smaller one, then the LDS digit planes, the plane
    sets and one plane set again -- three kernels, three pitches, one grow-only buffer -- and a smaller inventory."""
    e = engines(0)
    sh = Shard(8192 + 777, 5, "plain")
    sh.load(e)
    big = mostly_ones_batch(257)
    o_mask, _ = oracle.fit_mask(sh.res, sh.labels, *big)
    assert np.unpackbits(o_mask.view(np.uint8)).sum() > 0.95 * 257 * sh.res.shape[1]
    step(e, sh, "planes", *big)
    step(e, sh, "planes", *mostly_ones_batch(17))
    step(e, sh, "lds_any", *make_batch("many", 130, 21))
    step(e, sh, "plane_sets", *make_batch("needs70", 257, 23))
    step(e, sh, "planes", *make_batch("cfg5", 65, 25))
    step(e, sh, "lds_any", *make_batch("many", 17, 27))
    small = Shard(777, 29, "neg")
    small.load(e)
    step(e, small, "planes", *big)
    step(e, small, "lds_any", *make_batch("many", 65, 31))


def test_one_context_many_batches_blocks(engines):
    """Every path and bit 5: NODE_BLOCKS (one plane set), ROWS (LDS digit planes), NODE_TILES (70 needs: neither the
    LDS path, nor block-major plane sets, nor the coded path hold them), in turn and back."""
    e = engines(1 | 2 | 4 | 16 | 32 | 64)
    sh = Shard(8192 + 777, 33, "plain")
    sh.load(e)
    step(e, sh, "blocks_any", *mostly_ones_batch(257))
    step(e, sh, "lds_any", *make_batch("many", 65, 35))
    step(e, sh, "tiles_any", *make_batch("needs70", 130, 37))
    step(e, sh, "blocks_any", *make_batch("cfg5", 17, 39))
    step(e, sh, "tiles_any", *make_batch("needs70", 257, 41))
    step(e, sh, "lds_any", *make_batch("many", 130, 43))
    small = Shard(500, 45, "removed")
    small.load(e)
    step(e, small, "blocks_any", *mostly_ones_batch(130))
    step(e, small, "tiles_any", *make_batch("needs70", 71, 47))


def test_one_context_many_batches_bands(engines):
    """The coded and compare paths alone: JOB_BITS and NODE_TILES in turn, large batch first."""
    e = engines(1 | 2 | 4)
    sh = Shard(1500, 49, "plain")
    sh.load(e)
    zeros = (np.zeros((257, 4), dtype=np.int64), np.zeros(257, dtype=np.uint32))
    step(e, sh, "coded_any", *zeros)                                     # every bit of every valid pair set
    step(e, sh, "coded_any", *make_batch("chain", 65, 51))
    step(e, sh, "tiles_any", *make_batch("needs70", 130, 53))
    step(e, sh, "coded_any", *make_batch("chain", 17, 55))
    small = Shard(500, 57, "neg")
    small.load(e)
    step(e, small, "coded_any", *make_batch("chain", 130, 59))
    step(e, small, "tiles_any", *make_batch("needs70", 71, 61))


# ---------------------------------------------------------------- staged runs through the held pointer

@pytest.mark.parametrize("path", ["i64", "swar", "planes", "planes_blocks", "plane_sets", "lds2"])
def test_staged_runs_write_the_held_buffer(engines, path):
    """After pe_fit_mask the inventory changes four ways; every pe_fit_mask_run, with no new upload, writes the buffer
    the pointer obtained before names.  A different pe_fit_mask afterwards may move it: the new pointer is read."""
    bits, kind = PATHS[path][0], PATHS[path][4]
    e = engines(bits)
    N, J = 8192 + 777, 130
    inv = synth.make_inventory(N, 63, 0.4)
    inv.labels[::5] |= B17
    e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    m = Model.of(inv)
    req, need = make_batch(kind, J, 65)
    counts = counted(e, path, e.fit_mask, req, need)
    ptr = e.mask_ptr
    first = check_image(e, m.res, m.labels, req, need, counts, is_planes(path), ptr)

    def rerun():
        counted(e, path, e.fit_mask_run)
        return check_image(e, m.res, m.labels, req, need, None, is_planes(path), ptr)

    # a placement
    batch = synth.make_jobs(150, 13, "mixed")
    pods, _ = e.place_batch(batch)
    w_pods, _, _ = m.place(batch)
    np.testing.assert_array_equal(pods, w_pods)
    placed = rerun()
    assert (placed != first).any()
    # pe_release_gangs: the first 60 gangs give back what they hold
    gangs = GL.of_batch(batch, pods).only(range(60))
    back = GL.release(m.res, m.res0, np.zeros(N, dtype=bool), gangs)
    assert back.node < 0 and back.pods > 0
    assert e.release_gangs(*gangs.arrays()) == back.pods
    m.res = back.res
    np.testing.assert_array_equal(e.read_residuals(), m.res)
    released = rerun()
    assert (released != placed).any()
    # pe_update_nodes with removals
    deltas = make_deltas(N, 500, 17)
    e.update_nodes(*deltas)
    m.update(deltas)
    assert len(removed_slots(deltas))
    updated = rerun()
    assert (updated != released).any()
    # pe_reset_residuals
    e.reset_residuals()
    m.reset()
    np.testing.assert_array_equal(e.read_residuals(), m.res)
    reset = rerun()
    assert (reset != updated).any()
    # another batch: the pointer the call returns now
    req2, need2 = make_batch(kind, 257, 67)
    counts2 = counted(e, path, e.fit_mask, req2, need2)
    check_image(e, m.res, m.labels, req2, need2, counts2, is_planes(path))


# ---------------------------------------------------------------- shards

@pytest.mark.parametrize("N", [2048, 1501])       # 1024 + 1024, and 750 + 751
@pytest.mark.parametrize("path", ["i32", "therm", "planes_blocks", "lds1"])
def test_shard_images(path, N):
    """Two shard contexts of one inventory: each image is in shard-local node numbering over its own range."""
    bits, kind = PATHS[path][0], PATHS[path][4]
    J = 130
    sh = Shard(N, 69 + N, "neg")
    req, need = make_batch(kind, J, 71)
    _, whole = oracle.fit_mask(sh.res, sh.labels, req, need)
    total = np.zeros(J, dtype=np.int64)
    for rank in range(2):
        e = Engine(0, fit_path_mask=bits, rank=rank, world_size=2, exchange=lambda b: b + b)
        sh.load(e)
        assert e.shard_range() == (N * rank // 2, N * (rank + 1) // 2)
        counts = counted(e, path, e.fit_mask, req, need)
        check_image(e, sh.res, sh.labels, req, need, counts, is_planes(path))
        total += counts
        e.close()
    np.testing.assert_array_equal(total, whole)
