"""pe_fit_explain on the GPU against the checker (tests/fit_explain.py): every cell of both outputs of every job
compared, nothing sampled.  No test provokes a fault: every refusal is an argument check that returns before any
launch."""
import ctypes

import numpy as np
import pytest

import fit_explain as X
import tree_capacity as TC
from placement import Engine, PlacementError, _abi, synth, PE_EXPLAIN_ANY

pytestmark = pytest.mark.gpu

P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


def synth_case(n, seed, jobs=300):
    inv = synth.make_inventory(n, seed)
    req, need = synth.make_fit_jobs(jobs, seed + n)
    return X.Case(f"synth{n}", inv.cap, inv.used, inv.labels & ~X.ISLAND, inv.island,
                  np.ascontiguousarray(req, dtype=np.int64), np.ascontiguousarray(need, dtype=np.uint32))


def load(e, case):
    e.load_nodes(case.cap, case.used, case.labels, case.island)
    if len(case.remove):
        e.update_nodes(case.remove, np.full(len(case.remove), _abi.PE_NODE_REMOVE, np.uint8))
    return case.reference()


def same(got, want, what=""):
    assert got.hist.dtype == np.int64 and got.hist.shape == want[0].shape
    np.testing.assert_array_equal(got.hist, want[0], err_msg=f"hist {what}")
    if got.near is not None:
        assert got.near.dtype == np.uint64 and got.near.shape == want[1].shape
        np.testing.assert_array_equal(got.near, want[1], err_msg=f"near {what}")


@pytest.fixture()
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case3000():
    c = synth_case(3000, 7)
    return c, X.explain(*c.reference(), c.req, c.need)


@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 8193])
def test_node_sizes(eng, n_nodes):
    c = synth_case(n_nodes, 7)
    res, lab = load(eng, c)
    want = X.explain(res, lab, c.req, c.need)
    same(eng.fit_explain(c.req, c.need), want)
    assert (want[0].sum(axis=1) == n_nodes).all()


@pytest.mark.parametrize("n_nodes", [257, 3000])
def test_record_counts(eng, n_nodes):
    """1 .. 300 distinct records: below, at and above the block fold (32 records) and the split over grid rows."""
    c = synth_case(n_nodes, 9)
    res, lab = load(eng, c)
    req, need = X.distinct_records(300, 5)
    want = X.explain(res, lab, req, need)
    assert (want[0][:, 1:] > 0).any() and (want[1] > 0).any()
    for S in (1, 31, 32, 33, 63, 64, 65, 127, 129, 300):
        got = eng.fit_explain(req[:S], need[:S])
        same(got, (want[0][:S], want[1][:S]), f"S={S}")


def test_threshold_inventories_with_removed_slots(eng):
    for c in X.threshold_cases():
        res, lab = load(eng, c)
        assert len(c.remove) == 2 and (res[0] == X.NEVER).sum() == 2
        want = X.explain(res, lab, c.req, c.need)
        got = eng.fit_explain(c.req, c.need)
        same(got, want, c.name)
        assert (got.live == len(lab) - 2).all()


def test_arena_and_near_edges(eng):
    for c in (X.arena(), X.near_edges(), X.worked_example()):
        res, lab = load(eng, c)
        same(eng.fit_explain(c.req, c.need), X.explain(res, lab, c.req, c.need), c.name)
    got = eng.fit_explain(c.req, c.need)
    assert got.message(0) == X.EXAMPLE_MESSAGE and got.near[0].tolist() == list(X.EXAMPLE_NEAR)
    c = X.near_edges()
    load(eng, c)
    near = {int(v) for v in eng.fit_explain(c.req, c.need).near.reshape(-1)}
    assert {1, 1 << 63, (1 << 64) - 2} <= near


def test_repeated_shapes_and_null_arguments(eng, case3000):
    c, want = case3000
    load(eng, c)
    for j in (0, 17, 299):
        same(eng.fit_explain(c.req[j:j + 1], c.need[j:j + 1]), (want[0][j:j + 1], want[1][j:j + 1]))
    got = eng.fit_explain(np.repeat(c.req[5:6], 1000, axis=0), np.repeat(c.need[5:6], 1000))
    same(got, (np.repeat(want[0][5:6], 1000, axis=0), np.repeat(want[1][5:6], 1000, axis=0)))
    idx = np.array([3, 9, 3, 3, 250, 9, 0, 250, 3], dtype=np.int64)
    same(eng.fit_explain(c.req[idx], c.need[idx]), (want[0][idx], want[1][idx]))
    # need NULL is need 0
    res, lab = c.reference()
    same(eng.fit_explain(c.req[:40]), X.explain(res, lab, c.req[:40], None))
    # near=False: out_near NULL, the counts alone
    got = eng.fit_explain(c.req, c.need, near=False)
    assert got.near is None
    same(got, want)
    # out_hist NULL: the near values alone; both NULL: nothing to do
    near = np.full((300, 4), 7, dtype=np.uint64)
    rc = eng.lib.pe_fit_explain(eng.h, 300, P(c.req), P(c.need), None, 0, 0, None, None, None, P(near))
    assert rc == 0
    np.testing.assert_array_equal(near, want[1])
    assert eng.lib.pe_fit_explain(eng.h, 300, P(c.req), P(c.need), None, 0, 0, None, None, None, None) == 0


def test_identities_with_fit_mask_and_gang_capacity(eng, case3000):
    c, want = case3000
    load(eng, c)
    got = eng.fit_explain(c.req, c.need)
    np.testing.assert_array_equal(got.fits, eng.fit_mask(c.req, c.need))
    np.testing.assert_array_equal(got.fits, eng.gang_capacity(c.req, c.need)[2])
    same(eng.fit_explain(c.req, c.need), want)      # and again behind the other calls


@pytest.mark.parametrize("n_nodes", [257, 1025])
@pytest.mark.parametrize("name", TC.TREES)
def test_domain_form_on_the_named_trees(eng, name, n_nodes):
    c, level_size, parent = X.tree_case(name, n_nodes)
    res, lab = load(eng, c)
    J = len(c.req)
    whole = X.explain(res, lab, c.req, c.need)
    for level in range(len(level_size)):
        dom = X.level_domains(c.island, level_size, parent, level)
        n_dom = level_size[level]
        jd = ((np.arange(J) * 7) % n_dom).astype(np.int32)
        jd[::5] = PE_EXPLAIN_ANY                                    # mixed with real domains in one call
        empty = sorted(set(range(n_dom)) - set(dom.tolist()))       # a domain without nodes, where the tree has one
        if empty:
            jd[1] = empty[0]
        want = X.explain(res, lab, c.req, c.need, dom, jd)
        got = eng.fit_explain(c.req, c.need, jd, level, level_size, parent)
        same(got, want, f"{name} level {level}")
        np.testing.assert_array_equal(got.hist[::5], whole[0][::5])
        if empty:
            assert not got.hist[1].any() and not got.near[1].any()
    # the leaf domains and the nodes in none add up to the unrestricted form
    dom = X.level_domains(c.island, level_size, parent, 0)
    total = np.zeros_like(whole[0])
    for k in sorted(set(dom.tolist()) - {X.NO_DOMAIN}):
        total += eng.fit_explain(c.req, c.need, np.full(J, k, np.int32), 0, level_size, parent, near=False).hist
    out = dom == X.NO_DOMAIN
    assert out.any()
    total += X.explain(res[:, out], lab[out], c.req, c.need)[0]
    np.testing.assert_array_equal(total, eng.fit_explain(c.req, c.need).hist)


def test_answers_follow_the_state(eng):
    c = synth_case(3000, 7, jobs=120)
    res, lab = load(eng, c)
    lab = lab.copy()
    removed = []

    def check(what):
        now = eng.read_residuals()
        now[:, removed] = X.NEVER
        same(eng.fit_explain(c.req, c.need), X.explain(now, lab, c.req, c.need), what)
        return now

    first = check("loaded")
    eng.place_batch(synth.make_jobs(60, 7, "mixed"))
    after = check("placed")
    assert (after != first).any()
    eng.update_nodes([5], [_abi.PE_NODE_SET], np.array([[1, 2, 3, 4]], dtype=np.int64), np.zeros((1, 4), dtype=np.int64),
                     np.array([3], dtype=np.uint32), np.array([-1], dtype=np.int32))
    lab[5] = 3
    assert check("set")[:, 5].tolist() == [1, 2, 3, 4]
    eng.update_nodes([9], [_abi.PE_NODE_REMOVE])
    lab[9] = 0
    removed.append(9)
    check("removed")
    assert (eng.fit_explain(c.req, c.need).live == 2999).all()
    eng.reset_residuals()
    check("reset")
    c2 = synth_case(1025, 11, jobs=120)
    res2, lab2 = load(eng, c2)
    same(eng.fit_explain(c2.req, c2.need), X.explain(res2, lab2, c2.req, c2.need), "reloaded")


def test_staged_fit_batch_and_stats_are_untouched(eng, case3000):
    c, want = case3000
    load(eng, c)
    eng.jobs_upload(c.req[:200], c.need[:200])
    eng.fit_mask_run()
    before = eng.fit_counts()
    stats = eng.stats()
    res0 = eng.read_residuals()
    other = X.distinct_records(90, 2)
    eng.fit_explain(*other)
    eng.fit_explain(*other, np.zeros(90, np.int32), 0, [3000], None)
    assert eng.stats() == stats
    np.testing.assert_array_equal(eng.read_residuals(), res0)
    eng.fit_mask_run()
    np.testing.assert_array_equal(eng.fit_counts(), before)
    np.testing.assert_array_equal(before, want[0][:200, 0])


@pytest.mark.parametrize("n_nodes,world", [(1025, 2), (1025, 3), (2, 3)])
def test_shards(n_nodes, world):
    c, level_size, parent = X.tree_case("racks32", n_nodes)
    res, lab = c.reference()
    dom = X.level_domains(c.island, level_size, parent, 1)
    jd = (np.arange(len(c.req)) % (level_size[1] + 1) - 1).astype(np.int32)
    want = (X.explain(res, lab, c.req, c.need), X.explain(res, lab, c.req, c.need, dom, jd))
    hist = [np.zeros_like(want[0][0]), np.zeros_like(want[0][0])]
    near = [np.zeros_like(want[0][1]), np.zeros_like(want[0][1])]
    empty = 0
    for r in range(world):
        s = Engine(0, rank=r, world_size=world, exchange=lambda b, w=world: b * w)
        s.load_nodes(c.cap, c.used, c.labels, c.island)
        b, e = s.shard_range()
        empty += b == e
        for i, args in enumerate(((), (jd, 1, level_size, parent))):
            got = s.fit_explain(c.req, c.need, *args)
            same(got, X.explain(res[:, b:e], lab[b:e], c.req, c.need, *((dom[b:e], jd) if args else ())), f"rank {r}")
            hist[i] += got.hist
            near[i] = np.where(near[i] == 0, got.near, np.where(got.near == 0, near[i], np.minimum(near[i], got.near)))
        s.close()
    for i in range(2):
        np.testing.assert_array_equal(hist[i], want[i][0])
        np.testing.assert_array_equal(near[i], want[i][1])
    assert (empty > 0) == (world > n_nodes)


def test_refusals_write_nothing(eng):
    c, level_size, parent = X.tree_case("racks32", 257)
    J = len(c.req)
    hist = np.full((J, 32), -9, dtype=np.int64)
    near = np.full((J, 4), 9, dtype=np.uint64)
    ls = np.array(level_size, dtype=np.int32)
    jd = np.zeros(J, dtype=np.int32)

    def call(req=c.req, jd=jd, level=0, n_levels=len(ls), ls=ls, par=parent, J=J):
        rc = eng.lib.pe_fit_explain(eng.h, J, P(req), P(c.need), P(jd), level, n_levels, P(ls), P(par), P(hist), P(near))
        assert (hist == -9).all() and (near == 9).all()
        return rc, eng.lib.pe_last_error(eng.h).decode()

    assert call()[0] == _abi.PE_ESTATE                         # before pe_load_nodes
    load(eng, c)
    assert call(J=-1)[0] == _abi.PE_EINVAL
    bad = c.req.copy()
    bad[7, 2] = -1
    bad[9, 0] = -5
    rc, msg = call(req=bad)
    assert rc == _abi.PE_EINVAL and "index 30" in msg           # 7 * 4 + 2
    rc, msg = call(req=bad, jd=None, n_levels=0, ls=None, par=None)
    assert rc == _abi.PE_EINVAL and "index 30" in msg
    for level in (-1, 3):
        assert call(level=level)[0] == _abi.PE_EINVAL
    for value, level in ((-2, 0), (level_size[0], 0), (level_size[1], 1), (1, 2)):
        d2 = jd.copy()
        d2[11:] = value
        rc, msg = call(jd=d2, level=level)
        assert rc == _abi.PE_EINVAL and "index 11" in msg, (value, level, msg)
    assert call(n_levels=0)[0] == _abi.PE_EINVAL and call(n_levels=5)[0] == _abi.PE_EINVAL
    assert call(ls=None)[0] == _abi.PE_EINVAL and call(par=None)[0] == _abi.PE_EINVAL
    big = ls.copy()
    big[1] = 65537
    rc, msg = call(ls=big)
    assert rc == _abi.PE_EINVAL and "index 1" in msg
    p2 = parent.copy()
    p2[4] = level_size[1]
    rc, msg = call(par=p2)
    assert rc == _abi.PE_EINVAL and "index 4" in msg
    with pytest.raises(PlacementError):
        eng.fit_explain(bad)
    # the hierarchy arguments are not read without job_domain; n_jobs == 0 is PE_OK and writes nothing
    assert call(jd=None, level=77, n_levels=-4, ls=None, par=None, J=0)[0] == 0
    rc = eng.lib.pe_fit_explain(eng.h, J, P(c.req), P(c.need), None, 77, -4, None, None, P(hist), P(near))
    assert rc == 0
    res, lab = c.reference()
    want = X.explain(res, lab, c.req, c.need)
    np.testing.assert_array_equal(hist, want[0])
    np.testing.assert_array_equal(near, want[1])


def test_chunk_seam_and_blocks_that_fold_several_times(eng):
    """The seams of DESIGN.md section 28 at the smallest sizes that reach them: 233 017 distinct records are one more
    than a launch's tables hold (two launches, the second of one record), and with two node blocks every block row
    owns 256 records, eight folds of 32.  The inventory is 1025 nodes tiled from 16 distinct rows in a permuted
    order; the expectation is computed on the distinct rows weighted by their multiplicity."""
    S = 233016 + 1
    base = synth.make_inventory(16, 3)
    rows, labels, weight = X.tiled(base.residual().T, base.labels, 1025, 4)
    c = X.from_rows("tiled", rows, labels, *X.distinct_records(S, 8))
    load(eng, c)
    want = X.explain(base.residual(), base.labels, c.req, c.need, weight=weight)
    assert (want[0].sum(axis=1) == 1025).all() and (want[0][:, 1:] > 0).any() and (want[1] > 0).any()
    same(eng.fit_explain(c.req, c.need), want)
    same(eng.fit_explain(c.req[-40:], c.need[-40:], near=False), (want[0][-40:], None))
