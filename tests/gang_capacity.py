"""Checker for pe_gang_capacity: the rule of include/placement.h restated with Python integers (numpy
object arrays, true `//`, no reciprocal), and the input builders the CPU and GPU tests share.

    cap(j, n) = 0                                                        if not fit(j, n)
              = min(CAP_MAX, min over d with req_d > 0 of res_d // req_d)   otherwise
    slots[j] = sum_n cap(j, n)    max_node[j] = max_n cap(j, n)    nodes[j] = #{n : cap(j, n) >= 1}

fit(j, n) = (labels[n] & need[j]) == need[j] and req_d <= res_d in all four dimensions (signed).
`labels` are the engine's labels: synth.island_labels applied (bit 31 = the node has an island)."""
import numpy as np

from placement import synth

CAP_MAX = 2**31 - 1
I63 = 2**63 - 1
GiB = 1 << 30


def capacity_matrix(res, labels, req, need=None):
    """[J][N] object array of cap(j, n)."""
    res = np.asarray(res)
    N = res.shape[1]
    res_o = [res[d].astype(object) for d in range(4)]
    lab = np.asarray(labels, dtype=np.uint32).astype(np.int64)
    req = np.asarray(req).reshape(-1, 4)
    J = req.shape[0]
    nd = np.zeros(J, dtype=np.int64) if need is None else np.asarray(need, dtype=np.uint32).astype(np.int64)
    out = np.empty((J, N), dtype=object)
    for j in range(J):
        fit = (lab & nd[j]) == nd[j]
        cap = np.full(N, CAP_MAX, dtype=object)
        for d in range(4):
            q = int(req[j, d])
            fit = fit & np.asarray(res_o[d] >= q, dtype=bool)
            if q > 0:
                cap = np.minimum(cap, res_o[d] // q)
        out[j] = np.where(fit, cap, 0)
    return out


def capacity(res, labels, req, need=None):
    """(slots int64[J], max_node int32[J], nodes int64[J]) of the rule."""
    m = capacity_matrix(res, labels, req, need)
    J, N = m.shape
    slots = np.array([int(sum(m[j])) for j in range(J)], dtype=np.int64)   # <= 2^24 * 2^31
    max_node = np.array([int(max(m[j])) if N else 0 for j in range(J)], dtype=np.int32)
    nodes = np.array([int(np.count_nonzero(m[j] >= 1)) for j in range(J)], dtype=np.int64)
    return slots, max_node, nodes


def cap_cell(res4, label, req4, need):
    """One cell in plain Python integers (the hand-checkable form)."""
    res4 = [int(x) for x in res4]
    req4 = [int(x) for x in req4]
    if (int(label) & int(need)) != int(need) or any(q > r for q, r in zip(req4, res4)):
        return 0
    return min([CAP_MAX] + [r // q for q, r in zip(req4, res4) if q > 0])


# ---------------------------------------------------------------- shared inputs

def divisors():
    """The divisor list of the arithmetic tests: 1, 2, 3, 10, 2^k, 2^k +- 1 (k <= 62), 10^18, 2^63 - 2,
    2^63 - 1, ascending."""
    d = {1, 2, 3, 10, 10**18, 2**63 - 2, 2**63 - 1}
    for k in range(1, 63):
        d.update((2**k, 2**k + 1, 2**k - 1))
    return sorted(d)


def edge_inventory(n=4096, seed=11):
    """cap [4][n] (used = 0): residuals of every bit length up to 2^63 - 1.  Half the cells are random
    values of a set bit length; the others sit on or just below a multiple of a divisor of the list."""
    rng = np.random.default_rng(seed)
    divs = divisors()
    cap = np.zeros((4, n), dtype=np.int64)
    for d in range(4):
        for i in range(n):
            bits = (i + 17 * d) % 64
            if bits == 0:
                v = 0
            elif (i // 64 + d) % 2 == 0:
                lo, hi = 1 << (bits - 1), (1 << bits) - 1
                v = lo + int(rng.integers(0, hi - lo + 1, dtype=np.uint64))
            else:
                q = divs[int(rng.integers(0, len(divs)))]
                k = max(1, ((1 << bits) - 1) // q)
                v = min(I63, k * q) - int(rng.integers(0, 2))
            cap[d, i] = v
    cap[:, n - 1] = I63
    labels = (rng.integers(0, 16, n).astype(np.uint32))
    island = np.where(rng.integers(0, 3, n) == 0, np.arange(n), -1).astype(np.int32)
    return cap, np.zeros_like(cap), labels, island


def edge_shapes(n=256, seed=12):
    """n request vectors drawn per dimension from the divisor list (or 0), small divisors favoured so
    that a fair share of the nodes fit, with a label need on some."""
    rng = np.random.default_rng(seed)
    divs = divisors()
    small = [x for x in divs if x < 1 << 20]
    req = np.zeros((n, 4), dtype=np.int64)
    for j in range(n):
        for d in range(4):
            u = int(rng.integers(0, 10))
            if u < 3:
                req[j, d] = 0
            elif u < 7:
                req[j, d] = small[int(rng.integers(0, len(small)))]
            else:
                req[j, d] = divs[int(rng.integers(0, len(divs)))]
    req[0] = [0, 0, 0, 0]
    req[1] = [1, 1, 1, 1]
    req[2] = [I63, 0, 0, 0]
    req[3] = [1, 0, 0, 0]
    need = np.where(rng.integers(0, 4, n) == 0, rng.integers(0, 16, n), 0).astype(np.uint32)
    need[:4] = 0
    return req, need


def special_inventory():
    """Five hand-checkable nodes: (cap, used, labels, island)."""
    cap = np.array([[5000, 8 * GiB, 4, 100 * GiB],     # 0 ordinary
                    [I63, I63, I63, I63],               # 1 the largest residuals
                    [7, 0, 3, 9],                       # 2 a zero dimension
                    [10, 10, 10, 10],                   # 3 over-committed in dim 2 (used 11)
                    [0, 0, 0, 0]], dtype=np.int64).T.copy()   # 4 empty
    used = np.zeros_like(cap)
    used[2, 3] = 11
    labels = np.array([1, 1, 0, 1, 0], dtype=np.uint32)
    island = np.array([0, -1, -1, 3, -1], dtype=np.int32)
    return cap, used, labels, island


# (request, need, expected cap per node of special_inventory) -- worked by hand
ISLAND = 1 << 31
SPECIAL_CASES = [
    ([0, 0, 0, 0], 0, [CAP_MAX, CAP_MAX, CAP_MAX, 0, CAP_MAX]),       # all-zero request; node 3 is negative
    ([5000, 8 * GiB, 4, 100 * GiB], 0, [1, I63 // (100 * GiB), 0, 0, 0]),   # req = res exactly -> 1
    ([5000, 8 * GiB, 5, 100 * GiB], 0, [0, I63 // (100 * GiB), 0, 0, 0]),   # req = res + 1 -> 0
    ([1, 1, 1, 1], 0, [4, CAP_MAX, 0, 0, 0]),                         # 2^63 - 1 over 1 saturates
    ([7, 0, 3, 9], 0, [1, CAP_MAX, 1, 0, 0]),                         # zero in request and residual
    ([2, 0, 1, 2], 0, [4, CAP_MAX, 3, 0, 0]),
    ([1, 1, 0, 1], 0, [5000, CAP_MAX, 0, 0, 0]),                      # node 3: dim 2 negative, req_2 = 0 -> 0
    ([1250, GiB, 1, 10 * GiB], 1, [4, I63 // (10 * GiB), 0, 0, 0]),   # label bit 0
    ([1250, GiB, 1, 10 * GiB], 1 | ISLAND, [4, 0, 0, 0, 0]),          # island nodes only
    ([I63, I63, I63, I63], 0, [0, 1, 0, 0, 0]),
    ([1, 1, 1, 1], 2, [0, 0, 0, 0, 0]),                               # a need no node satisfies
]


def greedy_shapes():
    """(request, need) of the greedy equivalences: ordinary groups (one with a zero dimension), sized
    so that the capacity of a 200-node synth inventory stays in the hundreds."""
    return [([16000, 64 * GiB, 0, 0], 0),
            ([8000, 32 * GiB, 2, 50 * GiB], 1),
            ([32000, 128 * GiB, 0, 100 * GiB], 0)]


def greedy_island_shapes():
    return [([4000, 16 * GiB, 1, 10 * GiB], 1 | ISLAND),
            ([8000, 64 * GiB, 2, 0], 1 | ISLAND)]


def greedy_inventory():
    return synth.make_inventory(200, 21)


def one_group_batch(count, req, need):
    """pe_place_greedy arguments of one job with one group of `count` pods."""
    return (np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([count], dtype=np.int32),
            np.array([req], dtype=np.int64), np.array([need], dtype=np.uint32))
