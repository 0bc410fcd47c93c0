"""Random CSR batches of the PodGroup aggregation, shared by its CPU and GPU tests (no GPU, no engine):
the fixed-dimension form (4 values per container, u8 flags = presence bits 0-3 | kind << 4) and the
key-table form (n_keys values, u32 flags = presence bits | kind << 16)."""
import numpy as np


def random_csr(J, seed, big=False):
    rng = np.random.default_rng(seed)
    ng = rng.integers(0, 5, J)
    jgo = np.concatenate([[0], np.cumsum(ng)]).astype(np.int32)
    G = int(jgo[-1])
    rep = rng.integers(-1, 40, G).astype(np.int32)
    rep[rng.random(G) < 0.05] = 2**31 - 1
    nc = rng.integers(0, 5, G)
    gco = np.concatenate([[0], np.cumsum(nc)]).astype(np.int32)
    C = int(gco[-1])
    hi = 2**62 if big else 2**40
    req = rng.integers(0, hi, (C, 4), dtype=np.int64)
    req[rng.random((C, 4)) < 0.3] = 0
    fl = (rng.integers(0, 16, C) | (rng.integers(0, 4, C) << 4)).astype(np.uint8)
    mm = rng.integers(-2, 60, J).astype(np.int32)
    return jgo, mm, rep, gco, req, fl


def random_keys_csr(J, n_keys, seed, big=False):
    """random_csr's structure with n_keys values per container and u32 flags (presence bits of the
    n_keys keys | kind << 16)."""
    jgo, mm, rep, gco, _, fl8 = random_csr(J, seed, big)
    rng = np.random.default_rng(seed + 1)
    C = int(gco[-1])
    hi = 2**62 if big else 2**40
    req = rng.integers(0, hi, (C, n_keys), dtype=np.int64)
    req[rng.random((C, n_keys)) < 0.3] = 0
    pres = rng.integers(0, 1 << n_keys, C, dtype=np.int64).astype(np.uint32)
    fl = pres | ((fl8.astype(np.uint32) >> 4) << 16)
    return jgo, mm, rep, gco, req, fl


def one_job_csr(n_groups, n_cont_per_group, seed):
    rng = np.random.default_rng(seed)
    jgo = np.array([0, n_groups], np.int32)
    rep = rng.integers(-1, 5, n_groups).astype(np.int32)
    gco = (np.arange(n_groups + 1) * n_cont_per_group).astype(np.int32)
    C = int(gco[-1])
    req = rng.integers(0, 2**30, (C, 4), dtype=np.int64)
    fl = (rng.integers(0, 16, C) | (rng.integers(0, 4, C) << 4)).astype(np.uint8)
    mm = np.array([int(rep.clip(0).sum()) // 2 + 1], np.int32)
    return jgo, mm, rep, gco, req, fl


def concat(parts):
    """Fixed-dimension CSR batches back to back."""
    jgo, mm, rep, gco, req, fl = [np.zeros(1, np.int32)], [], [], [np.zeros(1, np.int32)], [], []
    g_off = c_off = 0
    for p in parts:
        jgo.append(p[0][1:] + g_off)
        mm.append(p[1])
        rep.append(p[2])
        gco.append(p[3][1:] + c_off)
        req.append(p[4].reshape(-1, 4))
        fl.append(p[5])
        g_off += int(p[0][-1])
        c_off += int(p[3][-1])
    return (np.concatenate(jgo).astype(np.int32), np.concatenate(mm).astype(np.int32),
            np.concatenate(rep).astype(np.int32), np.concatenate(gco).astype(np.int32),
            np.concatenate(req).astype(np.int64), np.concatenate(fl).astype(np.uint8))
