"""pe_pg_min_resources_wide on the GPU: the int64 pass for the jobs that fit, the 128-bit kernel
(pg_agg_wide_kernel, one lane per (job, key) pair) for the jobs that do not.  Compared with the C oracle
(unflagged jobs, flags, presence, members) and the big-integer checker tests/wide_agg.py (flagged jobs,
limb for limb; validated against the oracle in tests/test_wide_agg_cpu.py) -- never with the engine
itself.  pe_stats.agg_wide_jobs proves which jobs the 128-bit kernel answered."""
import json
import os

import numpy as np
import pytest

import oracle
import wide_agg as WA
import wide_keys as W
from placement import V1, V2, Engine, PlacementError, _abi, wide_ints, wide_limbs
from test_gpu_agg import random_keys_csr
from test_gpu_parity import random_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, gpu_resource_name="nvidia.com/gpu")
    yield e
    e.close()


def wide_jobs(eng):
    return eng.stats()["agg_wide_jobs"]


def check_against(eng, mode, arrs, n_keys, hi=None, lo=None, req_ints=None):
    """One wide call on (arrs, optional limbs) against the oracle and the checker; -> the outputs.
    Unflagged jobs (checker flag 0) equal the C oracle bit for bit with out_hi the sign extension;
    flagged jobs equal the checker limb for limb; the stats count exactly the flagged jobs."""
    jgo, mm, rep, gco, req, fl = arrs
    before = wide_jobs(eng)
    if hi is None:
        got = eng.pg_min_resources_wide(mode, jgo, mm, rep, gco, req, fl)
        want = oracle.pg_min_resources_keys(mode, *arrs)
        flagged = np.flatnonzero(want[3])
        c_vals, c_pres, c_mem, c_flag = WA.agg(mode, jgo, mm, rep, gco, WA.ints(req), fl, n_keys, jobs=flagged)
        c_flag[want[3] == 0] = 0
        w_pres, w_mem = want[1], want[2]
    else:
        got = eng.pg_min_resources_wide(mode, jgo, mm, rep, gco, lo, fl, cont_req_hi=hi)
        c_vals, c_pres, c_mem, c_flag = WA.agg(mode, jgo, mm, rep, gco, req_ints, fl, n_keys)
        want = None
        w_pres, w_mem = c_pres, c_mem
    o_lo, o_hi, pres, mem, flag = got
    np.testing.assert_array_equal(flag, c_flag)
    np.testing.assert_array_equal(pres, w_pres)
    np.testing.assert_array_equal(mem, w_mem)
    assert wide_jobs(eng) - before == int((c_flag != 0).sum())
    un = c_flag == 0
    if want is not None:
        np.testing.assert_array_equal(o_lo[un].view(np.int64), want[0][un])
        np.testing.assert_array_equal(o_hi[un], want[0][un] >> 63)
    w_lo, w_hi = WA.limbs(c_vals)              # (flag-2 jobs: zeros)
    sel = np.ones(len(flag), bool) if want is None else ~un
    np.testing.assert_array_equal(o_lo[sel], w_lo[sel])
    np.testing.assert_array_equal(o_hi[sel], w_hi[sel])
    return got


# ------------------------------------------------------------------ 1. pass-through

@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("n_keys", [1, 5, 16])
@pytest.mark.parametrize("J", [1, 300, 9000])
def test_wide_pass_through(eng, mode, n_keys, J):
    """No wide job: out_lo is pe_pg_min_resources_keys' answer bit for bit, out_hi its sign extension,
    every flag 0, and the 128-bit kernel did not run."""
    arrs = list(random_keys_csr(J, n_keys, 80 + J + n_keys + mode))
    arrs[4] = arrs[4] >> 12                     # < 2^28: x 2^31 replicas x 16 records stays int64
    want = oracle.pg_min_resources_keys(mode, *arrs)
    assert not want[3].any()
    before = wide_jobs(eng)
    o_lo, o_hi, pres, mem, flag = eng.pg_min_resources_wide(mode, *arrs, allow_overflow=False)
    assert wide_jobs(eng) == before
    np.testing.assert_array_equal(o_lo.view(np.int64), want[0])
    np.testing.assert_array_equal(o_hi, want[0] >> 63)
    if mode == V2 and J >= 300:
        assert (o_hi == -1).any()               # negative replica counts: negative sums
    np.testing.assert_array_equal(pres, want[1])
    np.testing.assert_array_equal(mem, want[2])
    assert not flag.any()
    k_out = eng.pg_min_resources_keys(mode, *arrs)
    np.testing.assert_array_equal(o_lo.view(np.int64), k_out[0])
    # the same batch with a zero hi limb given: still no wide job
    lo = arrs[4].astype(np.uint64)
    g2 = eng.pg_min_resources_wide(mode, *arrs[:4], lo, arrs[5], cont_req_hi=np.zeros_like(lo), allow_overflow=False)
    assert wide_jobs(eng) == before
    for a, b in zip(g2, (o_lo, o_hi, pres, mem, flag)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 2. mixed

@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("n_keys", WA.MIXED_KEYS)
@pytest.mark.parametrize("J", WA.MIXED_J)
def test_wide_mixed(eng, mode, n_keys, J):
    """About 1 % of the jobs overflow int64, on every call path of the int64 pass (kernel arguments,
    one latency launch, chunked, multi-range planner) and every kernel width."""
    arrs, picked, want = WA.mixed_batch(J, n_keys, mode)
    o_lo, o_hi, pres, mem, flag = check_against(eng, mode, arrs, n_keys)
    assert set(np.unique(flag)) <= {0, 1} and flag.any()
    np.testing.assert_array_equal(flag, want[3])


@pytest.mark.parametrize("mode", [V1, V2])
def test_wide_every_job(eng, mode):
    arrs, picked, want = WA.mixed_batch(300, 5, mode, every=True)
    _, _, _, _, flag = check_against(eng, mode, arrs, 5)
    assert flag.sum() > 30


# ------------------------------------------------------------------ 3. golden

def test_wide_golden(eng, golden_dir):
    """wide_keys.json through the wide call: every case equals its `want`, including the overflow case
    (5e18 + 1 per pod x 2 pods), which is flagged 1 and is 10000000000000000002."""
    with open(os.path.join(golden_dir, "wide_keys.json")) as f:
        g = json.load(f)

    def agg(mode, *arrs):
        lo, hi, pres, mem, flag = eng.pg_min_resources_wide(mode, *arrs, allow_overflow=False)
        return wide_ints(lo, hi), pres, mem, flag

    for mode, cases, flat in ((W.V1, g["v1"], W.v1_flat(g["v1"])), (W.V2, g["v2"], W.v2_flat(g["v2"]))):
        res, members, ovf, raw = W.run(agg, mode, flat)
        for j, case in enumerate(cases):
            want = case["want"] if mode == W.V1 else case["want"]["minResources"]
            assert ovf[j] == int(case.get("overflow", False)), case["name"]
            assert W.same(res[j], W.want_list(want)), (case["name"], res[j])
    assert cases[-1].get("overflow") and ovf[-1] == 1
    assert res[-1] == {"example.com/huge": 10000000000000000002}


# ------------------------------------------------------------------ 4. wide inputs

@pytest.mark.parametrize("mode", [V1, V2])
def test_wide_inputs_hand_built(eng, mode):
    """Two-limb inputs: the hand-built jobs of wide_agg.WIDE_CASES against the values worked out by hand
    there (2^127 - 1 exact, -2^127 exact, carries, the init-container rule in the hi limb, overhead after
    the max, the V1 min_member cut).  Without the jobs built to leave 128 bits the call is PE_OK."""
    (jgo, mm, rep, gco, req, fl), cases = WA.wide_case_batch(mode, with_flag2=False)
    lo, hi = wide_limbs(req)
    before = wide_jobs(eng)
    o_lo, o_hi, pres, mem, flag = eng.pg_min_resources_wide(mode, jgo, mm, rep, gco, lo, fl, cont_req_hi=hi,
                                                            allow_overflow=False)
    vals = wide_ints(o_lo, o_hi)
    for j, (name, _, _, want, want_flag) in enumerate(cases):
        assert flag[j] == want_flag, name
        assert vals[j].tolist() == want, (name, vals[j])
    assert wide_jobs(eng) - before == int((flag != 0).sum())
    check_against(eng, mode, (jgo, mm, rep, gco, req, fl), 2, hi=hi, lo=lo, req_ints=req)


@pytest.mark.parametrize("mode", [V1, V2])
def test_wide_inputs_leaving_128_bits(eng, mode):
    """With the jobs built to leave [-2^127, 2^127): those are flagged 2 with values 0, the call returns
    PE_EOVERFLOW with every output written, and the other jobs keep their exact answers."""
    (jgo, mm, rep, gco, req, fl), cases = WA.wide_case_batch(mode, with_flag2=True)
    lo, hi = wide_limbs(req)
    with pytest.raises(PlacementError) as ei:
        eng.pg_min_resources_wide(mode, jgo, mm, rep, gco, lo, fl, cont_req_hi=hi, allow_overflow=False)
    assert ei.value.code == _abi.PE_EOVERFLOW and "128-bit overflow in job" in str(ei.value)
    o_lo, o_hi, pres, mem, flag = check_against(eng, mode, (jgo, mm, rep, gco, req, fl), 2, hi=hi, lo=lo, req_ints=req)
    vals = wide_ints(o_lo, o_hi)
    for j, (name, _, _, want, want_flag) in enumerate(cases):
        assert flag[j] == want_flag, name
        assert vals[j].tolist() == ([0, 0] if want is None else want), (name, vals[j])
    assert (flag == 2).sum() == sum(c[4] == 2 for c in cases)


@pytest.mark.parametrize("mode", [V1, V2])
def test_wide_input_job_between_ordinary_jobs(eng, mode):
    """One job holds a wide input, its neighbours are ordinary: they equal the keys call and the oracle,
    and only that job went through the 128-bit kernel."""
    arrs, j_wide, lo, hi = WA.neighbours_batch(mode)
    before = wide_jobs(eng)
    o_lo, o_hi, pres, mem, flag = check_against(eng, mode, arrs, 5, hi=hi, lo=lo, req_ints=WA.ints(lo, hi))
    want = oracle.pg_min_resources_keys(mode, *arrs)
    others = np.arange(len(flag)) != j_wide
    assert flag[j_wide] == 1
    np.testing.assert_array_equal(flag[others], want[3][others])
    ok = others & (want[3] == 0)
    np.testing.assert_array_equal(o_lo[ok].view(np.int64), want[0][ok])
    np.testing.assert_array_equal(o_lo[ok].view(np.int64), eng.pg_min_resources_keys(mode, *arrs)[0][ok])
    assert wide_jobs(eng) - before == 1 + int(want[3][others].sum())


# ------------------------------------------------------------------ 5. shapes of the sub-batch

@pytest.mark.parametrize("mode", [V1, V2])
def test_wide_oversized_jobs(eng, mode):
    for arrs in WA.oversized_batches():
        _, _, _, _, flag = check_against(eng, mode, arrs, 4)
        assert flag.any()


def test_wide_interleaved_calls(eng):
    """Wide calls between keys calls and fixed-dimension calls of different sizes: the sub-batch
    buffers grow and are reused, the int64 pass's flag generations advance."""
    sizes = [1, 5000, 3, 300, 20000]
    wide_sizes = [1, 8193, 33, 40000, 257, 32, 8192, 1, 300, 8193]
    for i in range(10):
        mode = V1 if i % 2 else V2
        arrs, _, _ = WA.mixed_batch(wide_sizes[i], WA.MIXED_KEYS[i % 5], mode)
        check_against(eng, mode, arrs, WA.MIXED_KEYS[i % 5])
        k = random_keys_csr(sizes[i % 5], 5, 600 + i, big=(i % 3 == 0))
        for a, b in zip(eng.pg_min_resources_keys(mode, *k), oracle.pg_min_resources_keys(mode, *k)):
            np.testing.assert_array_equal(a, b)
        f = random_csr(sizes[(i + 2) % 5], 700 + i)
        for a, b in zip(eng.pg_min_resources(mode, *f), oracle.pg_min_resources(mode, *f)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 6. errors

def test_wide_errors(eng):
    """PE_EINVAL for a hi limb with bit 63, a negative lo without hi, n_keys 0 and 17, a presence bit
    past n_keys; after each error a correct call still answers."""
    arrs, _, _ = WA.mixed_batch(33, 5, V2)
    jgo, mm, rep, gco, req, fl = arrs

    def still_answers():
        check_against(eng, V2, arrs, 5)

    lo = req.astype(np.uint64)
    hi = np.zeros_like(lo)
    hi[7, 3] = 1 << 63
    with pytest.raises(PlacementError) as ei:
        eng.pg_min_resources_wide(V2, jgo, mm, rep, gco, lo, fl, cont_req_hi=hi)
    assert ei.value.code == _abi.PE_EINVAL and f"index {7 * 5 + 3}" in str(ei.value)
    still_answers()
    neg = req.copy()
    neg[4, 1] = -1
    with pytest.raises(PlacementError) as ei:
        eng.pg_min_resources_wide(V2, jgo, mm, rep, gco, neg, fl)
    assert ei.value.code == _abi.PE_EINVAL and f"index {4 * 5 + 1}" in str(ei.value)
    still_answers()
    for nk in (0, 17):
        with pytest.raises(PlacementError) as ei:
            eng.pg_min_resources_wide(V2, jgo, mm, rep, gco, np.zeros((len(fl), nk), np.int64), fl & 0xFFFF0000)
        assert ei.value.code == _abi.PE_EINVAL and "n_keys" in str(ei.value)
        still_answers()
    bad = fl.copy()
    bad[9] |= 1 << 5
    for h in (None, np.zeros_like(lo)):
        with pytest.raises(PlacementError) as ei:
            eng.pg_min_resources_wide(V2, jgo, mm, rep, gco, req if h is None else lo, bad, cont_req_hi=h)
        assert ei.value.code == _abi.PE_EINVAL and "cont_flags[9]" in str(ei.value)
        still_answers()
