"""pe_release_gangs / pe_assume_gangs on the device against tests/gang_ledger.py's checker: after every call the
residuals read back from the device are compared with the checker cell by cell, and the pod count with its count."""
import ctypes

import numpy as np
import pytest

import domain_placement as DP
import gang_ledger as GL
import gang_preempt as GP
import oracle
from placement import PE_NODE_REMOVE, PE_NODE_SET, Engine, PlacementError, _abi, synth

pytestmark = pytest.mark.gpu

GiB = DP.GiB
GRID_PASS = 256 * 256                # pe_kernels.h LG_THREADS x LG_MAX_BLOCKS: records one pass of the grid takes
R, A = GL.RELEASE, GL.ASSUME


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def load(e, p):
    e.load_nodes(p.cap, p.used, p.labels, p.island)
    return p.book()


def call(e, op, gangs):
    return (e.release_gangs if op == R else e.assume_gangs)(*gangs.arrays())


REFUSAL = [""]                       # the engine's message of the last refusal agree() saw


def agree(e, book, op, gangs, lo=None, hi=None):
    """The call on the engine and on the book, whichever way the checker decides: both let it through with the same
    pods and residuals, or both refuse it at the same node and the engine changes nothing.  Returns the outcome."""
    before = e.read_residuals()
    want = book.apply(op, gangs)
    if want.node < 0:
        assert call(e, op, gangs) == want.pods
    else:
        with pytest.raises(PlacementError) as ei:
            call(e, op, gangs)
        assert ei.value.code == _abi.PE_EINVAL and str(ei.value).endswith(f"at node {want.node}"), str(ei.value)
        assert ("more is given back than was taken" if op == R else "the pods do not fit") in str(ei.value)
        REFUSAL[0] = str(ei.value)
        assert np.array_equal(e.read_residuals(), before)
    assert np.array_equal(e.read_residuals(), book.visible()[:, lo:hi])
    return want


# ---------------------------------------------------------------- sizes and shapes

@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_sizes(eng, n):
    """A placement made by the C oracle greedy is assumed onto a fresh load and released again."""
    p = GL.greedy_placement(n, n_jobs=3 if n == 1 else 40)
    book = load(eng, p)
    out = GL.check_engine(eng, book, A, p.gangs())
    assert out.pods == int((p.pods >= 0).sum()) and np.array_equal(eng.read_residuals(), p.res_after)
    GL.check_engine(eng, book, R, p.gangs())
    assert np.array_equal(eng.read_residuals(), p.residual())
    assert n == 1 or out.pods > 0


@pytest.mark.parametrize("touched", [0, 1, 255, 256, 257, GRID_PASS + 1])
def test_touched_node_counts(eng, touched):
    n = max(touched, 1) + 3
    inv = synth.make_inventory(n, 19)
    eng.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    book = GL.Book(inv.cap, inv.used)
    nodes = np.random.default_rng(touched).permutation(n)[:touched]
    gangs = GL.spread_gangs(nodes, [3, 5, 0, 7])
    assert len(gangs.touched()) == touched
    assert GL.check_engine(eng, book, A, gangs).pods == touched
    assert touched == 0 or not np.array_equal(book.res, book.snap)
    assert GL.check_engine(eng, book, R, gangs).pods == touched
    assert np.array_equal(eng.read_residuals(), inv.residual())


def test_100000_zero_request_pods_and_real_pods_on_one_node(eng):
    cap = np.array([[64000] * 8, [256 * GiB] * 8, [8] * 8, [0] * 8], dtype=np.int64)
    eng.load_nodes(cap, np.zeros_like(cap), np.full(8, 1, dtype=np.uint32), np.arange(8, dtype=np.int32))
    book = GL.Book(cap, np.zeros_like(cap))
    gangs = GL.make_gangs([[([0, 0, 0, 0], [3] * 100000), ([1000, GiB, 1, 0], [3] * 5)], [([500, 0, 1, 0], [3, 4, 3])]])
    assert GL.check_engine(eng, book, A, gangs).pods == 100008
    assert eng.read_residuals()[:, 3].tolist() == [64000 - 6000, 251 * GiB, 1, 0]
    assert GL.check_engine(eng, book, R, gangs).pods == 100008
    assert np.array_equal(eng.read_residuals(), cap)


# ---------------------------------------------------------------- the identities after every placement call

def place_greedy(e, p):
    return e.place_batch(p.batch)


def place_domains(e, p):
    b = p.batch
    return e.place_greedy_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, *p.extra)


def place_first_fit(e, p):
    b = p.batch
    return e.place_first_fit_domains(b.job_group_off, b.priority, b.group_count, b.group_req, b.group_need, *p.extra)[:2]


@pytest.mark.parametrize("how", ["greedy_walk", "greedy_full_scan", "domains", "first_fit"])
def test_identities(how):
    e = Engine(0, greedy_flags=2 if how == "greedy_full_scan" else 0)
    p, place = {"greedy_walk": (lambda: GL.greedy_placement(1025), place_greedy),
                "greedy_full_scan": (lambda: GL.greedy_placement(1025), place_greedy),
                "domains": (lambda: GL.domain_placement("racks32", 1025), place_domains),
                "first_fit": (lambda: GL.first_fit_placement("racks32", 1025), place_first_fit)}[how]
    p = p()
    book = load(e, p)
    before = e.read_residuals()
    stats = e.stats()
    pods, st = place(e, p)
    assert np.array_equal(pods, p.pods) and np.array_equal(st, p.status) and (pods >= 0).any()
    after = e.read_residuals()
    assert np.array_equal(after, p.res_after)
    book.placed(after)
    counters = e.stats()
    gangs = GL.of_batch(p.batch, pods)
    # the placement followed by a release of its own arguments and outputs: bit-equal to before
    GL.check_engine(e, book, R, gangs)
    assert np.array_equal(e.read_residuals(), before)
    # release then assume is the identity
    GL.check_engine(e, book, A, gangs)
    assert np.array_equal(e.read_residuals(), after)
    # a reset followed by an assume of the same placement: what the placement left
    e.reset_residuals()
    book.reset()
    assert np.array_equal(e.read_residuals(), before)
    GL.check_engine(e, book, A, gangs)
    assert np.array_equal(e.read_residuals(), after)
    # assume then release is the identity
    GL.check_engine(e, book, R, gangs)
    assert np.array_equal(e.read_residuals(), before)
    # the same placement again from the released state: the same answer -- every path saw the new residuals
    pods2, st2 = place(e, p)
    assert np.array_equal(pods2, pods) and np.array_equal(st2, st) and np.array_equal(e.read_residuals(), after)
    # the new calls add to no counter
    now = e.stats()
    for k in ("pods_placed", "jobs_placed", "jobs_failed"):
        assert now[k] - counters[k] == counters[k] - stats[k], k
    e.close()


def test_staged_fit_batch_follows_the_release(eng):
    p = GL.greedy_placement(1025)
    book = load(eng, p)
    req, need = synth.make_fit_jobs(100, 7)
    eng.jobs_upload(req, need)
    eng.fit_mask_run()
    mask0, counts0 = oracle.fit_mask(p.residual(), p.labels, req, need)
    assert np.array_equal(eng.fit_counts(), counts0)
    pods, _ = eng.place_batch(p.batch)
    book.placed(eng.read_residuals())
    eng.fit_mask_run()
    mask1, counts1 = oracle.fit_mask(p.res_after, p.labels, req, need)
    assert np.array_equal(eng.fit_counts(), counts1) and not np.array_equal(counts0, counts1)
    half = p.gangs().only(range(0, len(p.gangs()), 2))
    out = GL.check_engine(eng, book, R, half)
    eng.fit_mask_run()                                      # the batch staged before the release, not uploaded again
    mask2, counts2 = oracle.fit_mask(out.res, p.labels, req, need)
    assert np.array_equal(eng.fit_counts(), counts2) and np.array_equal(eng.fit_mask_rows(0, 100), mask2)
    assert not np.array_equal(counts2, counts1)
    GL.check_engine(eng, book, A, half)
    eng.fit_mask_run()
    assert np.array_equal(eng.fit_counts(), counts1) and np.array_equal(eng.fit_mask_rows(0, 100), mask1)


def test_calls_after_a_release_equal_a_fresh_engine(eng):
    """Capacity, gang_fit_domains and place_greedy after a release see what an engine loaded with the checker's
    residuals sees."""
    p = GL.domain_placement("racks32", 1025)
    book = load(eng, p)
    pods, _ = place_domains(eng, p)
    book.placed(eng.read_residuals())
    gangs = GL.of_batch(p.batch, pods)
    out = GL.check_engine(eng, book, R, gangs.only(range(0, len(gangs), 2)))
    assert (out.res >= 0).all()
    fresh = Engine(0)
    fresh.load_nodes(out.res, np.zeros_like(out.res), p.labels, p.island)
    req, need = synth.make_fit_jobs(60, 11)
    for a, b in zip(eng.gang_capacity(req, need), fresh.gang_capacity(req, need)):
        assert np.array_equal(a, b)
    job_domain, level, sizes, parent = p.extra
    b = p.batch
    J = len(job_domain)
    pj = np.repeat(np.arange(J, dtype=np.int32), 2)
    pd = np.stack([job_domain, (np.asarray(job_domain) + 1) % sizes[level]], axis=1).astype(np.int32).reshape(-1)
    fit_args = (b.job_group_off, b.group_count, b.group_req, b.group_need, pj, pd, level, sizes, parent)
    got, want = eng.gang_fit_domains(*fit_args), fresh.gang_fit_domains(*fit_args)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    jobs = synth.make_jobs(40, 13, "mixed")
    for x, y in zip(eng.place_batch(jobs), fresh.place_batch(jobs)):
        assert np.array_equal(x, y)
    assert np.array_equal(eng.read_residuals(), fresh.read_residuals())
    fresh.close()


def test_one_context_walked_beside_the_checker(eng):
    p = GL.domain_placement("racks32", 257)
    job_domain, level, sizes, parent = p.extra
    book = load(eng, p)

    def place():
        want = DP.place(eng.read_residuals(), p.labels, p.island, p.batch, job_domain, level, sizes, parent)
        pods, st = place_domains(eng, p)
        assert np.array_equal(pods, want[0]) and np.array_equal(st, want[1]) and np.array_equal(eng.read_residuals(), want[2])
        book.placed(want[2])
        return GL.of_batch(p.batch, pods)

    gangs = place()
    GL.check_engine(eng, book, R, gangs)                    # place, release
    again = place()                                         # place again: the same pods
    assert np.array_equal(again.pod_node, gangs.pod_node)
    holds = []                                              # per gang: the nodes on which it holds something
    for v in range(len(gangs)):
        one = gangs.only([v])
        holds.append({int(n) for g in range(len(one.group_count)) if one.group_req[g].any()
                      for n in one.pod_node[DP.pod_offsets(one.group_count)[g]:DP.pod_offsets(one.group_count)[g + 1]] if n >= 0})
    first = next(v for v in range(len(gangs)) if holds[v])
    GL.check_engine(eng, book, R, gangs.only([first]))      # one gang released ...
    x = min(holds[first])
    cap_x = p.cap[:, x]
    used_x = cap_x - book.res[:, x]                         # ... and the informer reports its node as it is now
    eng.update_nodes([x], [PE_NODE_SET], [cap_x], [used_x], [int(p.labels[x])], [int(p.island[x])])
    book.node_set(x, cap_x, used_x)
    assert np.array_equal(eng.read_residuals(), book.visible())
    out = agree(eng, book, A, gangs.only([first]))          # the released gang may come back onto the updated node
    assert out.node < 0
    out = agree(eng, book, R, gangs.only([first]))          # ... and go again: the snapshot is the node as reported
    assert out.node < 0
    other = next(v for v in range(len(gangs)) if v != first and holds[v] and x not in holds[v])
    y = min(holds[other])
    used_y = p.cap[:, y] - book.res[:, y]                   # a node set with a gang still on it folds the gang into `used`
    eng.update_nodes([y], [PE_NODE_SET], [p.cap[:, y]], [used_y], [int(p.labels[y])], [int(p.island[y])])
    book.node_set(y, p.cap[:, y], used_y)
    out = agree(eng, book, R, gangs.only([other]))          # ... and the release of it is refused
    assert out.node >= 0
    third = next(v for v in range(len(gangs)) if holds[v] and not holds[v] & {x, y} and v not in (first, other))
    z = min(holds[third])
    eng.update_nodes([z], [PE_NODE_REMOVE])
    book.node_remove(z)
    out = agree(eng, book, R, gangs.only([third]))          # pods on a removed slot count nothing
    assert out.node < 0 and out.pods < sum(1 for s in gangs.only([third]).pod_node if s >= 0)
    eng.reset_residuals()
    book.reset()
    assert np.array_equal(eng.read_residuals(), book.visible())
    rest = [v for v in range(len(gangs)) if v not in (first, other, third)]
    agree(eng, book, A, gangs.only(rest))                   # reset, assume
    agree(eng, book, A, gangs.only([other]))                # whatever the checker says of the folded node, so says the engine
    book = load(eng, p)                                     # reload, assume: the residuals the placement left
    GL.check_engine(eng, book, A, gangs)
    assert np.array_equal(eng.read_residuals(), p.res_after)


def victims_as_gangs(vic):
    return GL.Gangs(vic.group_off, vic.group_count, vic.group_req, vic.pod_node)


def test_preempt_answer_carried_out_on_one_engine(eng):
    """The victims are assumed onto an inventory that does not hold them yet, so the engine's residuals are the
    preempt case's; then the answered set is released and the job fits, one victim fewer of a prefix answer and it
    does not; assumed back, the residuals are the start's."""
    pc = GP.tree_pcase("racks32", 257, 0)
    c, all_vic = pc.case, victims_as_gangs(pc.vic)
    none = np.zeros(c.cap.shape[1], dtype=bool)
    free = GL.release(c.residual(), c.cap, none, all_vic)   # the inventory without the victims
    assert free.node < 0
    eng.load_nodes(c.cap, c.cap - free.res, c.labels, c.island)
    book = GL.Book(c.cap, c.cap - free.res)
    GL.check_engine(eng, book, A, all_vic)
    start = eng.read_residuals()
    assert np.array_equal(start, c.residual())
    pre = eng.gang_preempt_domains(*pc.call_args())
    b = c.batch
    tried = 0
    for p in np.nonzero(pre.prefix >= 1)[0][:6]:
        lst = [int(v) for v in pc.pair_vic[int(pc.pair_vic_off[p]):int(pc.pair_vic_off[p + 1])]]
        one = (b.job_group_off, b.group_count, b.group_req, b.group_need, [int(pc.pair_job[p])], [int(pc.pair_domain[p])],
               c.level, c.level_size, c.parent)
        for victims, fits in ((GP.final_set(pc.pair_vic_off, pc.pair_vic, p, pre.victims[p]), 1),
                              (lst[:int(pre.prefix[p]) - 1], 0)):
            gangs = all_vic.only(victims)
            GL.check_engine(eng, book, R, gangs)
            assert eng.gang_fit_domains(*one).fits.tolist() == [fits], (int(p), victims)
            GL.check_engine(eng, book, A, gangs)
            assert np.array_equal(eng.read_residuals(), start)
        tried += 1
    assert tried > 0


# ---------------------------------------------------------------- refusals

SENTINEL = 77
FNS = ("pe_release_gangs", "pe_assume_gangs")


def raw(e, fn, off, cnt, req, pod, n_gangs=None, out=True):
    conv = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)   # noqa: E731
    keep = [conv(off, np.int32), conv(cnt, np.int32), conv(req, np.int64), conv(pod, np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    n = n_gangs if n_gangs is not None else len(keep[0]) - 1
    pods = ctypes.c_int64(SENTINEL)
    rc = getattr(e.lib, fn)(e.h, n, *[ptr(a) for a in keep], ctypes.byref(pods) if out else None)
    return rc, e.lib.pe_last_error(e.h).decode(), pods.value


def test_refusals():
    n = 300
    inv = synth.make_inventory(n, 71)
    e = Engine(0)
    Q = [1000, 2 * GiB, 0, 0]
    good = dict(off=[0, 1, 2], cnt=[2, 1], req=np.array([Q, [500, GiB, 0, 0]], dtype=np.int64), pod=[5, -1, 299])
    for fn in FNS:
        rc, msg, pods = raw(e, fn, **good)                  # before a load
        assert rc == _abi.PE_ESTATE and "no inventory" in msg and pods == SENTINEL
    e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    # something is out, so that both a release and an assume of `good` go through
    assert e.assume_gangs(**{"gang_group_off": good["off"], "group_count": good["cnt"], "group_req": good["req"],
                             "pod_node": good["pod"]}) == 2
    before = e.read_residuals()
    stats = e.stats()

    def refused(text, fns=FNS, **change):
        for fn in fns:
            rc, msg, pods = raw(e, fn, **dict(good, **change))
            assert rc == _abi.PE_EINVAL and text in msg, (fn, rc, msg, change)
            assert pods == SENTINEL and np.array_equal(e.read_residuals(), before)

    refused("n_gangs < 0", n_gangs=-1)
    refused("n_gangs outside", n_gangs=2**31)
    refused("gang_group_off is NULL", off=None, n_gangs=2)
    refused("not rising from 0 at index 0", off=[1, 1, 2])
    refused("not rising from 0 at index 2", off=[0, 2, 1])
    refused("group_count or group_req is NULL", cnt=None)
    refused("group_count or group_req is NULL", req=None)
    refused("group_count: negative value at index 1", cnt=[2, -1])
    refused("group_req: negative value in group at index 0", req=np.array([[1, 1, -1, 0], Q], dtype=np.int64))
    refused("pod_node is NULL", pod=None)
    refused("pod_node: value outside [-1, n_total) at index 2", pod=[5, -1, 300])
    refused("pod_node: value outside [-1, n_total) at index 0", pod=[-2, -1, 299])
    # one unit more than was taken, on one node in one dimension
    refused("more is given back than was taken", fns=FNS[:1], req=np.array([Q[:3] + [1], [500, GiB, 0, 0]], dtype=np.int64))
    refused("at node 299", fns=FNS[:1], req=np.array([Q, [501, GiB, 0, 0]], dtype=np.int64))
    # the excess only visible as a total over two gangs: node 299 holds 500, each gang gives 300 back
    refused("at node 299", fns=FNS[:1], off=[0, 1, 2], cnt=[1, 1], req=np.array([[300, 0, 0, 0]] * 2, dtype=np.int64), pod=[299, 299])
    free = int(before[0][7])
    refused("the pods do not fit", fns=FNS[1:], off=[0, 1], cnt=[1], req=np.array([[free + 1, 0, 0, 0]], dtype=np.int64), pod=[7])
    refused("at node 7", fns=FNS[1:], off=[0, 1, 2], cnt=[1, 1],
            req=np.array([[free // 2 + 1, 0, 0, 0]] * 2, dtype=np.int64), pod=[7, 7])
    # k x req past int64: 4 x 2^62 wraps to 0 and would pass every bound
    refused("at node 9", off=[0, 1], cnt=[4], req=np.array([[1 << 62, 0, 0, 0]], dtype=np.int64), pod=[9, 9, 9, 9])
    # a zero-sum dimension is not looked at, the others are: the good call goes through both ways, without out_pods too
    for fn in FNS[::-1]:
        rc, msg, pods = raw(e, fn, **good)
        assert rc == _abi.PE_OK and pods == 2, msg
    assert raw(e, FNS[1], out=False, **good)[0] == _abi.PE_OK and raw(e, FNS[0], out=False, **good)[0] == _abi.PE_OK
    # no gangs, and gangs without pods
    for fn in FNS:
        assert raw(e, fn, None, None, None, None, n_gangs=0)[::2] == (_abi.PE_OK, 0)
        assert raw(e, fn, [0, 1], [0], np.array([Q], dtype=np.int64), None)[::2] == (_abi.PE_OK, 0)
    assert np.array_equal(e.read_residuals(), before) and e.stats() == stats
    e.close()


def test_negative_snapshot_in_a_dimension_the_call_does_not_move(eng):
    cap = np.array([[1000, 1000], [GiB, GiB], [0, 0], [5, 5]], dtype=np.int64)
    used = np.array([[0, 0], [0, 0], [0, 0], [9, 0]], dtype=np.int64)      # node 0: cap - used = -4 in storage
    eng.load_nodes(cap, used, np.ones(2, dtype=np.uint32), np.full(2, -1, dtype=np.int32))
    book = GL.Book(cap, used)
    g = GL.make_gangs([[([100, 1, 0, 0], [0, 0, 1])]])
    assert agree(eng, book, A, g).node < 0 and eng.read_residuals()[:, 0].tolist() == [800, GiB - 2, 0, -4]
    assert agree(eng, book, R, g).node < 0
    assert agree(eng, book, A, GL.make_gangs([[([0, 0, 0, 1], [1, 0])]])).node == 0
    assert agree(eng, book, R, GL.make_gangs([[([0, 0, 0, 1], [0])]])).node == 0


# ---------------------------------------------------------------- sharded contexts

@pytest.mark.parametrize("world", [2, 3])
def test_sharded_contexts(world):
    n = 1025                                                # uneven shards: 512 + 513, or 341 + 342 + 342
    inv = synth.make_inventory(n, 29)
    ranks = [Engine(0, rank=r, world_size=world, exchange=lambda b, w=world: b * w) for r in range(world)]
    for e in ranks:
        e.load_nodes(inv.cap, inv.used, inv.labels, inv.island)
    bounds = [e.shard_range() for e in ranks]
    assert bounds[0][0] == 0 and bounds[-1][1] == n and len({hi - lo for lo, hi in bounds}) > 1
    edges = [x for lo, hi in bounds for x in (lo, hi - 1)]  # the first and the last node of every shard
    nodes = edges + [int(x) for x in np.random.default_rng(world).permutation(n)[:200]] + edges[::-1]
    gangs = GL.spread_gangs(nodes, [700, 3 * GiB, 0, 11], per_gang=5)
    books = [GL.Book(inv.cap, inv.used) for _ in ranks]
    for op in (A, R, A):
        for e, book, (lo, hi) in zip(ranks, books, bounds):
            out = GL.check_engine(e, book, op, gangs, lo, hi)
            assert out.pods == len(nodes)
    # every rank holds the whole mirror: a second assume of one pod per edge node that only the FIRST left room for
    # is decided alike everywhere, and so is a release of more than is out
    tight = GL.make_gangs([[([int(books[0].res[0][x]), 0, 0, 0], [x]) for x in edges]])
    for e, book, (lo, hi) in zip(ranks, books, bounds):
        assert agree(e, book, A, tight, lo, hi).node < 0
    msgs = set()
    for e, book, (lo, hi) in zip(ranks, books, bounds):
        assert agree(e, book, A, GL.make_gangs([[([1, 0, 0, 0], [edges[-1]])]]), lo, hi).node == edges[-1]
        msgs.add(REFUSAL[0])
    assert len(msgs) == 1 and "the pods do not fit" in msgs.pop()
    over = GL.make_gangs([[([1, 0, 0, 0], [edges[2]])], [([int(books[0].snap[0][edges[1]]) + 1, 0, 0, 0], [edges[1]])]])
    msgs = set()
    for e, book, (lo, hi) in zip(ranks, books, bounds):
        assert agree(e, book, R, over, lo, hi).node == edges[1]
        msgs.add(REFUSAL[0])
    assert len(msgs) == 1 and "more is given back" in msgs.pop()
    for e, book, (lo, hi) in zip(ranks, books, bounds):
        assert agree(e, book, R, tight, lo, hi).node < 0
        assert agree(e, book, R, gangs, lo, hi).node < 0
        assert np.array_equal(e.read_residuals(), inv.residual()[:, lo:hi])
        e.close()
