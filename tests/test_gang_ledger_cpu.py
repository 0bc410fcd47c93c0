"""The rule of pe_release_gangs / pe_assume_gangs on the CPU (tests/gang_ledger.py): the three identities through real
placements by the C oracle greedy, domain_placement.place and first_fit.place_first_fit on the named trees, the
refusals, the cells the rule does not look at, and the bindings against the header.  No GPU."""
import inspect
import re

import numpy as np
import pytest

import gang_ledger as GL
import tree_capacity as TC
from placement import Engine, _abi

I64_MAX = 2**63 - 1


def identities(p):
    """The three identities on one placement; returns the pods that counted."""
    before, gangs = p.residual(), p.gangs()
    none = np.zeros(before.shape[1], dtype=bool)
    # 1) the placement followed by a release of its own arguments and outputs: the residuals before it
    out = GL.release(p.res_after, before, none, gangs)
    assert out.node < 0 and np.array_equal(out.res, before)
    placed = int((np.asarray(p.pods) >= 0).sum())
    assert out.pods == placed
    # 2) a reset followed by an assume of the same placement: the residuals the placement left
    back = GL.assume(before, before, none, gangs)
    assert back.node < 0 and back.pods == placed and np.array_equal(back.res, p.res_after)
    # 3) release then assume, and assume then release, are the identity
    again = GL.assume(out.res, before, none, gangs)
    assert again.node < 0 and np.array_equal(again.res, p.res_after)
    assert np.array_equal(GL.release(back.res, before, none, gangs).res, before)
    # ... gang by gang, in reverse order, as well as all at once
    res = p.res_after
    for v in reversed(range(len(gangs))):
        res = GL.release(res, before, none, gangs.only([v])).res
    assert np.array_equal(res, before)
    return placed


@pytest.mark.parametrize("n", [257, 1025])
def test_identities_after_the_greedy(n):
    p = GL.greedy_placement(n)
    assert identities(p) > 0 and (p.status == 1).any() and (p.status == 0).any()


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [257, 1025])
def test_identities_after_a_domain_placement(name, n):
    p = GL.domain_placement(name, n)
    assert identities(p) > 0 and (p.status == 0).any()


@pytest.mark.parametrize("name", TC.TREES)
@pytest.mark.parametrize("n", [257, 1025])
def test_identities_after_a_first_fit(name, n):
    p = GL.first_fit_placement(name, n)
    assert identities(p) > 0 and (p.status == 0).any()


def test_an_unschedulable_job_counts_nothing():
    p = GL.greedy_placement(257)
    failed = [int(j) for j in np.nonzero(p.status == 1)[0]]
    assert failed
    only = p.gangs().only(failed)
    assert (only.pod_node == -1).all() and len(only.pod_node) > 0
    none = np.zeros(257, dtype=bool)
    for op in (GL.RELEASE, GL.ASSUME):
        out = GL.apply(op, p.res_after, p.residual(), none, only)
        assert out.node < 0 and out.pods == 0 and np.array_equal(out.res, p.res_after)


def two_nodes():
    snap = np.array([[10, 10], [8, 8], [4, 4], [0, -6]], dtype=np.int64)      # node 1: cap - used < 0 in storage
    res = np.array([[6, 7], [8, 5], [4, 2], [0, -6]], dtype=np.int64)         # taken: n0 {4,0,0,0}, n1 {3,3,2,0}
    return res, snap, np.zeros(2, dtype=bool)


def test_one_unit_too_many_is_refused():
    res, snap, none = two_nodes()
    ok = GL.make_gangs([[([4, 0, 0, 0], [0]), ([3, 3, 2, 0], [1])]])
    out = GL.release(res, snap, none, ok)
    assert out.node < 0 and out.pods == 2 and np.array_equal(out.res, snap)
    for d in range(3):                                      # one unit more on node 1 in one dimension
        q = [3, 3, 2, 0]
        q[d] += 1
        out = GL.release(res, snap, none, GL.make_gangs([[([4, 0, 0, 0], [0]), (q, [1])]]))
        assert out == GL.Outcome(None, -1, 1)
    # assume: node 1 holds {7, 5, 2}; one unit more in one dimension does not fit
    assert GL.assume(res, snap, none, GL.make_gangs([[([7, 5, 2, 0], [1])]])).res[:, 1].tolist() == [0, 0, 0, -6]
    for d in range(3):
        q = [7, 5, 2, 0]
        q[d] += 1
        assert GL.assume(res, snap, none, GL.make_gangs([[([6, 0, 0, 0], [0]), (q, [1])]])) == GL.Outcome(None, -1, 1)


def test_excess_visible_only_as_a_total_over_two_gangs():
    res, snap, none = two_nodes()
    a, b = [([2, 2, 1, 0], [1])], [([2, 2, 1, 0], [1])]     # each fits what node 1 misses ({3, 3, 2}), both do not
    assert GL.release(res, snap, none, GL.make_gangs([a])).node < 0 and GL.release(res, snap, none, GL.make_gangs([b])).node < 0
    assert GL.release(res, snap, none, GL.make_gangs([a, b])) == GL.Outcome(None, -1, 1)
    a, b = [([4, 0, 0, 0], [1, 0])], [([4, 0, 0, 0], [1])]  # assume: 7 cpu on node 1 hold one pod of 4, not two
    assert GL.assume(res, snap, none, GL.make_gangs([a])).node < 0 and GL.assume(res, snap, none, GL.make_gangs([b])).node < 0
    assert GL.assume(res, snap, none, GL.make_gangs([a, b])) == GL.Outcome(None, -1, 1)


def test_a_dimension_the_call_does_not_move_may_be_negative():
    res, snap, none = two_nodes()
    g = GL.make_gangs([[([1, 1, 0, 0], [1, 1])]])           # storage on node 1 is -6 of -6 and is not asked about
    out = GL.assume(res, snap, none, g)
    assert out.node < 0 and out.res[:, 1].tolist() == [5, 3, 2, -6]
    assert np.array_equal(GL.release(out.res, snap, none, g).res, res)
    # ... but a single unit of it is refused either way: 0 more fits, and nothing was taken
    g = GL.make_gangs([[([0, 0, 0, 1], [1])]])
    assert GL.assume(res, snap, none, g).node == 1 and GL.release(res, snap, none, g).node == 1


def test_removed_and_skipped_slots_count_nowhere():
    res, snap, _ = two_nodes()
    removed = np.array([True, False])
    g = GL.make_gangs([[([100, 100, 100, 100], [0, 0, -1]), ([1, 1, 1, 0], [-1, 1, -1])], [([9, 9, 9, 9], [-1, -1])]])
    out = GL.release(res, snap, removed, g)
    assert out.node < 0 and out.pods == 1 and out.res[:, 0].tolist() == res[:, 0].tolist()
    assert out.res[:, 1].tolist() == [8, 6, 3, -6]
    out = GL.assume(res, snap, removed, g)
    assert out.node < 0 and out.pods == 1 and out.res[:, 1].tolist() == [6, 4, 1, -6]


def test_a_product_past_int64_is_refused_not_wrapped():
    snap = np.array([[I64_MAX], [0], [0], [0]], dtype=np.int64)
    res = np.array([[0], [0], [0], [0]], dtype=np.int64)
    none = np.zeros(1, dtype=bool)
    g = GL.make_gangs([[([1 << 62, 0, 0, 0], [0, 0, 0, 0])]])           # 4 x 2^62 = 2^64: 0 in 64 bits
    assert GL.release(res, snap, none, g) == GL.Outcome(None, -1, 0)
    assert GL.assume(snap, snap, none, g) == GL.Outcome(None, -1, 0)
    g = GL.make_gangs([[([I64_MAX - 5, 0, 0, 0], [0]), ([5, 0, 0, 0], [0])]])
    assert GL.release(res, snap, none, g).res[0][0] == I64_MAX and GL.assume(snap, snap, none, g).res[0][0] == 0


def test_book_follows_node_updates():
    res, snap, _ = two_nodes()
    book = GL.Book(snap, np.zeros_like(snap))
    book.res = res.copy()
    g = GL.make_gangs([[([3, 3, 2, 0], [1])]])
    book.node_set(1, [7, 5, 2, 0], [0, 0, 0, 6])           # the informer folds the placement into `used`
    assert book.apply(GL.RELEASE, g).node == 1              # ... and the release of it is refused
    book.node_remove(1)
    assert book.apply(GL.RELEASE, g).pods == 0 and book.visible()[0][1] == np.iinfo(np.int64).min


# ---------------------------------------------------------------- the bindings

def header_decl(name):
    text = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["pe_release_gangs", "pe_assume_gangs"])
def test_binding_matches_the_header(name):
    args = header_decl(name)
    assert args == ["pe_ctx* ctx", "int64_t n_gangs", "const int32_t* gang_group_off", "const int32_t* group_count",
                    "const int64_t* group_req", "const int32_t* pod_node", "int64_t* out_pods"]
    res, argtypes = _abi.SIGNATURES[name]
    P, i64 = _abi.P, _abi.i64
    assert res is _abi.ctypes.c_int and argtypes[:6] == [P, i64, P, P, P, P] and len(argtypes) == len(args)
    assert argtypes[6] is _abi.ctypes.POINTER(i64)
    assert hasattr(_abi.load(), name)
    method = getattr(Engine, name[3:])
    assert list(inspect.signature(method).parameters) == ["self", "gang_group_off", "group_count", "group_req", "pod_node"]


def test_header_states_the_rule():
    text = " ".join(open(_abi.HEADER).read().split())
    text = text.replace(" * ", " ")
    for needle in ("more is given back than was taken", "the pods do not fit", "labels, group needs and the best-fit rule are not consulted",
                   "bit-equal to those before it", "PE_NODE_SET of a node folds the placements on it",
                   "the calls work with world_size > 1"):
        assert needle in text, needle
    assert re.search(r"#define PE_ABI_VERSION 7\b", text)
