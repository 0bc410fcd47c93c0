"""pe_drain_move_domains against the rule in Python integers: candidates in ascending c, each by drain_fit.py's statement
on the residuals as the earlier fitting ones left them, every other candidate node a removed slot, the give-backs last."""
import numpy as np
import pytest

import drain_fit as DF
from placement import Engine, _abi, synth

pytestmark = pytest.mark.gpu

LDS, NEVER, gpus = 1016, DF.NEVER, DF.gpus              # pe_kernels.h PL_LDS_NODES
RACKS = 6      # 0: the segment, 1: worked example, 2: candidates only, 3: one candidate, 4: rack 0's sources, 5: the story


def rule(res, labels, island, book, cand_node, cand_domain, level_size, cordon=True):
    """(fits, moved, fail_slot, target, residual [4][N]); cordon=False: only the candidate's own node is out."""
    R, C, g_of = np.array(res, dtype=np.int64, copy=True), len(cand_node), book.group_of_slot()
    fits, moved = np.ones(C, dtype=np.uint8), np.zeros(C, dtype=np.int64)
    fail, target = np.full(C, -1, dtype=np.int64), np.full(len(book.pod), -1, dtype=np.int32)
    for c in range(C):
        Rc = R.copy()
        if cordon:
            Rc[:, [int(n) for n in cand_node if n != cand_node[c]]] = NEVER
        f, m, fl, t = DF.drain_python(Rc, labels, island, book, cand_node[c:c + 1], cand_domain[c:c + 1], 0, level_size, None)
        fits[c], moved[c], fail[c] = f[0], m[0], fl[0]
        for s in np.nonzero(t >= 0)[0]:                                  # a candidate that fits stands
            target[s] = t[s]
            R[:, t[s]] -= book.req[g_of[s]]
    for c in np.nonzero(fits)[0]:                                        # the give-backs, afterwards
        if R[0][cand_node[c]] != NEVER:
            for s in np.nonzero(book.pod == cand_node[c])[0]:
                R[:, cand_node[c]] += book.req[g_of[s]]
    return fits, moved, fail, target, R


def batch_case(size, seed=11):
    """(free GPUs per node, island, book, cand_node, cand_domain, gone, names) -- ids shuffled.  Rack 0 has `size` nodes;
    33 candidates drain into it, 2 of them its own nodes (size >= 3), the rest nodes of rack 4.  Its first node X is the
    one candidate of rack 3.  Racks 1, 2 and 5 are fixed."""
    N = size + 3 + 2 + 2 + 33 + 10
    ids = [int(x) for x in np.random.default_rng(seed).permutation(N)]
    take = lambda k: [ids.pop() for _ in range(k)]
    r0, (A, B, Cn), (P, Q), (Y1, Y2), src, S = take(size), take(3), take(2), take(2), take(33), take(10)
    island, free = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int64)
    for rack, nodes in enumerate((r0, [A, B, Cn], [P, Q], [Y1, Y2], src, S)):
        island[nodes] = rack
    X, inside = r0[0], r0[1:3] if size >= 3 else []
    free[[r0[k * size // 24] for k in range(24)]] = [1 + k % 4 for k in range(24)]   # scarce, all over the segment
    free[inside] = 4                                                     # tempting, and cordoned
    free[[Cn, Y1, Y2]] = 4, 8, 8
    free[S] = [0, 3, 1, 4, 4, 0, 2, 2, 0, 2]
    gangs, cand = [], []
    into0 = list(inside) + src[:33 - len(inside)]
    for i, n in enumerate(into0):                                        # rack 0's 33: 1 to 3 pods of 1 to 4 GPUs each
        gangs.append([(gpus(1 + i % 4, 500 + i), 0, [n] * (1 + i % 3))])
    # the worked example; then a rack of candidates only: P's pod finds nobody, Q is a removed slot that holds a pod
    gangs += [[(gpus(3), 0, [A])], [(gpus(2), 0, [B])], [(gpus(1), 0, [P])], [(gpus(1), 0, [Q])]]
    # X, a node of rack 0, into rack 3: pods of two gangs, the second an island run of 2 x 3 GPUs among other nodes' pods
    gangs += [[(gpus(2), 0, [X, Y1, X])], [(gpus(3), DF.ISLAND, [X, -1, X]), (gpus(1), 0, [Y2])]]
    # the story, rack 5: S0's best fit is S1, a later candidate; S1's is S0, just drained; S5 (two gangs) takes S6 and S9
    # and fails on its third pod; S7 fits on exactly what came back; S8 fits nothing but the cordoned S7
    gangs += [[(gpus(3), 0, [S[0]])], [(gpus(3), 0, [S[1]])], [(gpus(2), 0, [S[5], S[5]])], [(gpus(5), 0, [S[5]])],
              [(gpus(2), 0, [S[7], S[7]])], [(gpus(2), 0, [S[8]])]]
    story = [(S[0], 5), (S[1], 5), (S[5], 5), (S[7], 5), (S[8], 5)]
    rest = [(A, 1), (B, 1), (P, 2), (Q, 2), (X, 3)]
    for i, n in enumerate(into0):                                        # the domains' candidates interleaved
        cand.append((n, 0))
        if i % 3 == 0 and i // 3 < len(story):
            cand += [story[i // 3], rest[i // 3]]
    node, dom = np.array([c[0] for c in cand], dtype=np.int32), np.array([c[1] for c in cand], dtype=np.int32)
    names = dict(A=A, B=B, C=Cn, P=P, Q=Q, X=X, Y1=Y1, Y2=Y2, S=S)
    return free, island, DF.make_book(gangs), node, dom, [Q], names


def load(eng, free, island, book, gone=()):
    """The inventory with the book assumed onto it, then `gone` removed: (labels, the residuals the call sees)."""
    N = len(free)
    res, labels = DF.flat_case(free).cap, synth.island_labels(np.ones(N, dtype=np.uint32), island)
    held = np.zeros_like(res)
    for s in np.nonzero(book.pod >= 0)[0]:
        held[:, book.pod[s]] += book.req[book.group_of_slot()[s]]
    eng.load_nodes(res + held, np.zeros_like(res), labels, island)
    eng.assume_gangs(book.off, book.cnt, book.req, book.pod)
    if len(gone):
        eng.update_nodes(list(gone), [1] * len(gone))
    now = eng.read_residuals()
    assert np.array_equal(np.delete(now, list(gone), axis=1), np.delete(res, list(gone), axis=1))
    return labels, now


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("size", [1, 255, 257, LDS - 1, LDS, LDS + 1])
def test_against_the_rule(eng, size):
    free, island, book, node, dom, gone, nm = batch_case(size)
    labels, before = load(eng, free, island, book, gone)
    want = rule(before, labels, island, book, node, dom, [RACKS])
    # the batch shows what it was made for, by the reference alone
    at = {int(n): c for c, n in enumerate(node)}
    S, fits, moved, loose = nm["S"], want[0], want[1], rule(before, labels, island, book, node, dom, [RACKS], cordon=False)
    assert np.bincount(dom, minlength=RACKS).tolist() == [33, 2, 2, 1, 0, 5]
    assert [int(fits[at[nm[k]]]) for k in "ABPQX"] == [1, 0, 0, 1, 1] and moved[at[nm["X"]]] == 4
    assert [int(fits[at[S[i]]]) for i in (0, 1, 5, 7, 8)] == [1, 1, 0, 1, 0] and moved[at[S[5]]] == 2
    assert loose[0][at[S[8]]] == 1                                       # S8 fails by the cordon alone
    into0 = dom == 0                                                     # rack 0 rolls back too, beyond one node
    assert size == 1 or (fits[into0].any() and ((fits[into0] == 0) & (moved[into0] > 0)).any())
    assert want[4][2][nm["X"]] == before[2][nm["X"]] + 10                # the give-back into another active domain
    stats = eng.stats()
    for dry in (True, False):                                            # the dry run, then the committed call
        got = eng.drain_move_domains(*book.args(), node, dom, 0, [RACKS], dry_run=dry)
        for name, g, w in zip(("fits", "moved", "fail_slot", "target"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (dry, name, np.nonzero(g != w)[0][:10].tolist())
        assert np.array_equal(eng.read_residuals(), before if dry else want[4])
        assert eng.stats() == stats
    # ledger closure: the moved slots released at their targets and assumed at their old nodes
    eng.release_gangs(book.off, book.cnt, book.req, want[3])
    eng.assume_gangs(book.off, book.cnt, book.req, np.where(want[3] >= 0, book.pod, -1))
    assert np.array_equal(eng.read_residuals(), before)


def test_identity_one_candidate_is_drain_fit_domains(eng):
    free, island, book, node, dom, gone, _ = batch_case(257)
    load(eng, free, island, book, gone)
    for c in np.nonzero(dom != 0)[0].tolist() + [0, 1]:
        want = eng.drain_fit_domains(*book.args(), node[c:c + 1], dom[c:c + 1], 0, [RACKS])
        got = eng.drain_move_domains(*book.args(), node[c:c + 1], dom[c:c + 1], 0, [RACKS], dry_run=True)
        assert DF.same(got, want), c


def test_refusals():
    free, island, book, node, dom, gone, nm = batch_case(3)
    twice, big = node.copy(), book.req.copy()
    twice[5], big[-1] = twice[0], gpus(3)                                # S8 gives back 3 of the 2 GPUs it took
    outs = [np.full(n, 77, dtype=t) for n, t in ((len(node), np.uint8), (len(node), np.int64), (len(node), np.int64),
                                                 (len(book.pod), np.int32))]

    def answers(e, code, text, node=node, req=book.req, flags=0):
        arrs = [book.off, book.cnt, req, book.need, book.pod, node, dom, np.array([RACKS], dtype=np.int32)]
        k = [np.ascontiguousarray(a).ctypes.data for a in arrs]
        rc = e.lib.pe_drain_move_domains(e.h, len(book.off) - 1, *k[:5], len(node), k[5], k[6], 0, 1, k[7], None, flags,
                                         *[x.ctypes.data for x in outs])
        msg = e.lib.pe_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg)
        assert all((x == 77).all() for x in outs) == (code != _abi.PE_OK)   # a refusal writes no output

    e = Engine(0)
    answers(e, _abi.PE_ESTATE, "no inventory")
    _, before = load(e, free, island, book, gone)
    answers(e, _abi.PE_EINVAL, "flags: unknown bits", flags=2)
    answers(e, _abi.PE_EINVAL, "cand_node: a node named twice at index 5", node=twice)
    answers(e, _abi.PE_EINVAL, "more than was taken (the residual would exceed the reset snapshot) at node %d" % nm["S"][8], req=big)
    assert np.array_equal(e.read_residuals(), before)
    for r in range(2):                                                   # a 2-shard context
        s = Engine(0, rank=r, world_size=2, exchange=lambda x: x * 2)
        s.load_nodes(np.full_like(before, 8), np.zeros_like(before), np.ones(len(free), dtype=np.uint32), island)
        answers(s, _abi.PE_EINVAL, "shard")
        s.close()
    answers(e, _abi.PE_OK, "", flags=1)                                  # the same arguments are accepted
    e.close()
