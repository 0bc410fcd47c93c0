"""The big-integer checker of the 128-bit aggregation (tests/wide_agg.py) against the C oracle, and the
batches the GPU tests of pe_pg_min_resources_wide use (tests/test_gpu_agg_wide.py): no GPU.

The checker is trusted for the values past int64 only because, on random key-table batches, it gives
the C oracle's value for every job the oracle does not flag and flags exactly the jobs the oracle flags."""
import json
import os

import numpy as np
import pytest

import oracle
import wide_agg as WA
import wide_keys as W
from placement import _abi, wide_ints, wide_limbs
from test_gpu_agg import random_keys_csr

V1, V2 = 1, 2


@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("n_keys", [1, 5, 16])
@pytest.mark.parametrize("big", [False, True])
def test_checker_equals_c_oracle(mode, n_keys, big):
    """Values, presence, members of every unflagged job; checker flag != 0 <=> oracle ovf == 1."""
    arrs = random_keys_csr(1500, n_keys, 11 + n_keys + mode, big=big)
    want, w_pres, w_mem, w_ovf = oracle.pg_min_resources_keys(mode, *arrs)
    got, pres, mem, flag = WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], n_keys)
    np.testing.assert_array_equal(flag != 0, w_ovf == 1)
    assert not (flag == 2).any()               # int64 inputs: the largest sum is far below 2^127
    if big:
        assert w_ovf.sum() > 10                # the flagged side is exercised
    np.testing.assert_array_equal(pres, w_pres)
    np.testing.assert_array_equal(mem, w_mem)
    ok = w_ovf == 0
    assert ok.sum() > 100
    np.testing.assert_array_equal(got[ok], want[ok].astype(object))


def test_limb_helpers_round_trip():
    vals = [[0, 1, 2**63], [2**64 - 1, 2**64, 2**127 - 1]]
    lo, hi = wide_limbs(vals)
    assert lo.dtype == np.uint64 and hi.dtype == np.uint64
    assert WA.ints(lo, hi) == vals
    signed = [[-1, -2**127, 2**127 - 1, -2**64, 5]]
    slo, shi = WA.limbs(signed)
    assert wide_ints(slo, shi).tolist() == signed
    with pytest.raises(ValueError):
        wide_limbs([-1])


def test_abi_declares_the_wide_call():
    """The entry point is exported with the header's arity and pe_stats ends in agg_wide_jobs."""
    lib = _abi.load()
    assert hasattr(lib, "pe_pg_min_resources_wide")
    assert len(_abi.SIGNATURES["pe_pg_min_resources_wide"][1]) == 16
    assert _abi.PeStats._fields_[-1][0] == "agg_wide_jobs"
    assert lib.pe_pg_min_resources_wide(None, 1, 0, 1, *([None] * 12)) == _abi.PE_EINVAL   # no context


def test_golden_overflow_case(golden_dir):
    """wide_keys.json through the checker: every case equals its `want`, the overflow case (5e18 + 1 per
    pod x 2 pods) is flagged 1 and is 10000000000000000002."""
    with open(os.path.join(golden_dir, "wide_keys.json")) as f:
        g = json.load(f)

    def agg(mode, jgo, mm, rep, gco, req, fl):
        vals, pres, mem, flag = WA.agg(mode, jgo, mm, rep, gco, WA.ints(req), fl, req.shape[1])
        assert not (flag == 2).any()
        return vals, pres, mem, flag

    n_ovf = 0
    for mode, cases, flat in ((V1, g["v1"], W.v1_flat(g["v1"])), (V2, g["v2"], W.v2_flat(g["v2"]))):
        res, members, ovf, _ = W.run(agg, mode, flat)
        for j, case in enumerate(cases):
            want = case["want"] if mode == V1 else case["want"]["minResources"]
            assert ovf[j] == int(case.get("overflow", False)), case["name"]
            assert W.same(res[j], W.want_list(want)), (case["name"], res[j])
            n_ovf += int(ovf[j])
    assert n_ovf == 1
    assert res[-1] == {"example.com/huge": 10000000000000000002}


@pytest.mark.parametrize("mode", [V1, V2])
def test_hand_built_cases_by_hand(mode):
    """The hand-built wide-input jobs: the checker gives the value worked out by hand in WIDE_CASES, and
    flag 2 exactly in the cases built to leave 128 bits."""
    (jgo, mm, rep, gco, req, fl), cases = WA.wide_case_batch(mode, with_flag2=True)
    vals, pres, mem, flag = WA.agg(mode, jgo, mm, rep, gco, req, fl, 2)
    assert len(cases) >= 3
    for j, (name, _, _, want, want_flag) in enumerate(cases):
        assert flag[j] == want_flag, name
        assert vals[j].tolist() == ([0, 0] if want is None else want), (name, vals[j])
    (jgo, mm, rep, gco, req, fl), cases = WA.wide_case_batch(mode, with_flag2=False)
    assert not (WA.agg(mode, jgo, mm, rep, gco, req, fl, 2)[3] == 2).any()
    lo, hi = wide_limbs(req)                   # every input travels as two limbs with hi < 2^63
    assert not (hi >> np.uint64(63)).any()


@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("n_keys", WA.MIXED_KEYS)
@pytest.mark.parametrize("J", WA.MIXED_J)
def test_mixed_batches_hold_no_flag2_job(J, n_keys, mode):
    """The mixed batches of the GPU test: at least one job flagged by the oracle, every flagged job has an
    exact 128-bit answer (checker flag 1), every other job is the oracle's."""
    arrs, picked, want = WA.mixed_batch(J, n_keys, mode)
    flagged = np.flatnonzero(want[3])
    assert len(flagged) >= 1 and len(picked) >= 1
    assert int(arrs[4].max(initial=0)) < 2**62
    _, _, _, flag = WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], n_keys, jobs=flagged)
    assert (flag[flagged] == 1).all()


@pytest.mark.parametrize("mode", [V1, V2])
def test_other_gpu_batches_hold_no_flag2_job(mode):
    arrs, picked, want = WA.mixed_batch(300, 5, mode, every=True)
    flagged = np.flatnonzero(want[3])
    assert len(picked) == 300 and len(flagged) > 30
    assert (WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], 5, jobs=flagged)[3][flagged] == 1).all()
    for arrs in WA.oversized_batches():
        w_ovf = oracle.pg_min_resources_keys(mode, *arrs)[3]
        flagged = np.flatnonzero(w_ovf)
        assert len(flagged) >= 1               # the oversized job is a wide one
        assert (WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], 4, jobs=flagged)[3][flagged] == 1).all()
    arrs, j_wide, lo, hi = WA.neighbours_batch(mode)
    vals, pres, mem, flag = WA.agg(mode, *arrs[:4], WA.ints(lo, hi), arrs[5], 5)
    want = oracle.pg_min_resources_keys(mode, *arrs)
    assert flag[j_wide] == 1 and not (flag == 2).any()
    others = np.arange(len(flag)) != j_wide
    np.testing.assert_array_equal(flag[others], want[3][others])
    ok = others & (want[3] == 0)
    np.testing.assert_array_equal(vals[ok], want[0][ok].astype(object))
