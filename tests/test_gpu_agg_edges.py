"""The int64 edges of the aggregation on the GPU (tests/agg_edges.py: jobs on both sides of every overflow
test of agg_job_t, on the grid of every request packing), down every call path: kernel arguments, one
pinned segment, one latency launch of 32- and 256-job segments, the chunked paths, the segment-size
override, the device-resident kernel, zero-copy chunks, an oversized job read in place, and the 128-bit
pass behind pe_pg_min_resources_wide with and without a high limb.

Unflagged jobs are compared with the C oracle; flagged jobs compare flags with both references and their
values, through the wide call, with the big-integer checker limb for limb; pe_stats.agg_wide_jobs moves
by exactly the flagged jobs; every case's hand-worked value is asserted on top.  Never the engine against
itself.  tests/test_agg_edges_cpu.py proves the references, the coverage and the packing on the CPU.

Packing is steered through the data (PE_AGG_WIDE and the other once-per-process knobs are not touched):
pe_stats.agg_narrow_segments == agg_segments for the narrowed batches and 0 for the unnarrowable ones
proves it on the chunked paths."""
import numpy as np
import pytest

import agg_edges as E
import oracle
import wide_agg as WA
from placement import V1, V2, Engine, wide_ints

pytestmark = pytest.mark.gpu

WIDTHS = [1, 4, 5, 8, 9, 16]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0, gpu_resource_name="nvidia.com/gpu")
    yield e
    e.close()


class Ref:
    """Both references of a batch, computed once: the C oracle's outputs and, for the jobs it flags, the
    checker's exact values."""

    def __init__(self, mode, arrs, n_keys):
        self.o = oracle.pg_min_resources_keys(mode, *arrs)
        flagged = np.flatnonzero(self.o[3])
        vals, pres, mem, flag = WA.agg(mode, *arrs[:4], WA.ints(arrs[4]), arrs[5], n_keys, jobs=flagged)
        assert (flag[flagged] == 1).all()                  # (no case leaves 128 bits)
        np.testing.assert_array_equal(pres[flagged], self.o[1][flagged])
        np.testing.assert_array_equal(mem[flagged], self.o[2][flagged])
        self.lo, self.hi = WA.limbs(vals)


def compare(eng, mode, arrs, n_keys, ref, rows=None, fixed=False, zero_hi=False):
    """The keys call and the wide call (and the fixed-dimension call) on arrs against ref[rows]."""
    rows = np.arange(len(arrs[0]) - 1) if rows is None else np.asarray(rows)
    want = [x[rows] for x in ref.o]
    for a, b in zip(eng.pg_min_resources_keys(mode, *arrs), want):
        np.testing.assert_array_equal(a, b)
    if fixed:
        f = (*arrs[:5], E.fixed_flags(arrs[5]))
        for a, b, c in zip(eng.pg_min_resources(mode, *f), oracle.pg_min_resources(mode, *f), want):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c)
    before = eng.stats()["agg_wide_jobs"]
    if zero_hi:
        lo = arrs[4].astype(np.uint64)
        out = eng.pg_min_resources_wide(mode, *arrs[:4], lo, arrs[5], cont_req_hi=np.zeros_like(lo))
    else:
        out = eng.pg_min_resources_wide(mode, *arrs)
    o_lo, o_hi, pres, mem, flag = out
    np.testing.assert_array_equal(flag, want[3])
    np.testing.assert_array_equal(pres, want[1])
    np.testing.assert_array_equal(mem, want[2])
    assert eng.stats()["agg_wide_jobs"] - before == int(want[3].sum())
    un = want[3] == 0
    np.testing.assert_array_equal(o_lo[un].view(np.int64), want[0][un])
    np.testing.assert_array_equal(o_hi[un], want[0][un] >> 63)
    np.testing.assert_array_equal(o_lo[~un], ref.lo[rows][~un])
    np.testing.assert_array_equal(o_hi[~un], ref.hi[rows][~un])
    return out


def by_hand(out, cases, pos):
    """The edge jobs' answers of a wide call against the values worked out by hand in the table."""
    o_lo, o_hi, pres, mem, flag = out
    vals = wide_ints(o_lo[pos], o_hi[pos])
    for i, c in enumerate(cases):
        got = (int(flag[pos[i]]), vals[i, c["key"]], int(mem[pos[i]]), bool(pres[pos[i]] >> c["key"] & 1))
        assert got == (c["flag"], c["want"], c["mem"], c["pres"]), (c["name"], c["key"], got)
        if c["want"] == -E.LIM:
            assert o_hi[pos[i], c["key"]] == -1 and o_lo[pos[i], c["key"]] == 1 << 63   # out_hi all ones


def variants(n_keys, rots):
    """(shifts of the keys | None = unnarrowable, keys that carry a table: key 0 and the last)."""
    keys = sorted({0, n_keys - 1})
    return [(None, keys)] + [(E.key_shifts(n_keys, r), keys) for r in rots]


def batch(mode, n_keys, sh, keys, J, seg_jobs, seed, pad=0, min_cont=0, with_big=True):
    """The edge jobs of (mode, sh) among J - n filler jobs, placed by lane -> (arrs, cases, pos, reached, full).
    With 256-job segments the filler holds a stretch of 512 small jobs (agg_edges.small_filler): random
    filler of the wider tables passes 48 KB long before 256 jobs, the stretch fills a segment at every
    width.  The lanes are those of the key-table calls; the fixed-dimension call on the same batch packs
    u8 flags, so its segments may end elsewhere where the byte limit ends them (agg_edges.assemble)."""
    edge, cases = E.edge_batch(mode, n_keys, sh, keys, pad=pad)
    small = E.small_filler(2 * E.SEG_JOBS, n_keys, seed + 1, sh) if seg_jobs == E.SEG_JOBS else None
    n = len(cases) + with_big + (2 * E.SEG_JOBS if small else 0)
    assert J > n
    filler = E.filler_batch(J - n, n_keys, seed, sh, min_cont)
    big = E.oversized_job(n_keys, sh) if with_big else None
    arrs, pos, reached, full = E.assemble(edge, filler, n_keys, seg_jobs, mode == V1, big=big, small=small)
    assert len(arrs[0]) - 1 == J
    return arrs, cases, pos, reached, full


# ------------------------------------------------------------------ one job per call

@pytest.mark.parametrize("no_karg", ["", "1"])
@pytest.mark.parametrize("n_keys", WIDTHS)
def test_edges_one_job_calls(eng, monkeypatch, n_keys, no_karg):
    """Every edge job alone: in the kernel arguments (<= 512 B), or with PE_AGG_NO_KARG=1 as one pinned
    segment; the 4-key table also through the fixed-dimension call (the u8 instance).  Which jobs fit the
    512 B -- at every width a job on each side of int64 of every step -- is asserted on the CPU
    (test_agg_edges_cpu.py::test_kernel_argument_route_is_taken); the others take the pinned segment."""
    if no_karg:
        monkeypatch.setenv("PE_AGG_NO_KARG", "1")
    for mode in (V1, V2):
        for sh, keys in variants(n_keys, range(len(E.SHIFTS)) if n_keys == 1 else (0, 2, 5)):
            edge, cases = E.edge_batch(mode, n_keys, sh, keys)
            ref = Ref(mode, edge, n_keys)
            for j in range(len(cases)):
                one = E.csr_slice(edge, j, j + 1)
                out = compare(eng, mode, one, n_keys, ref, rows=[j], fixed=n_keys == 4, zero_hi=j % 2 == 1)
                by_hand(out, cases[j:j + 1], np.array([0]))


# ------------------------------------------------------------------ one latency launch

@pytest.mark.parametrize("J", [33, 2048, 2049])
@pytest.mark.parametrize("n_keys", WIDTHS)
def test_edges_latency_launch(eng, n_keys, J):
    """One launch of several segments, the host waiting on the flag: 32-job segments up to 2048 jobs, 256-job
    segments from 2049 on; edge jobs at lane 0, at the last lane and directly after an oversized job.  The
    wide call runs with no high limb and with a zero one."""
    seg = 32 if J <= 2048 else E.SEG_JOBS
    for mode in (V1, V2):
        for sh, keys in variants(n_keys, (1, 4) if n_keys > 1 else (0, 3, 6)):
            if J == 33:       # three edge jobs per call: lane 0, lane 31, lane 0 of the second segment
                edge, cases = E.edge_batch(mode, n_keys, sh, keys)
                filler = E.filler_batch(30, n_keys, 21 + n_keys, sh)
                for a in range(0, len(cases) - 2, 3):
                    arrs, pos, reached, _ = E.assemble(E.csr_slice(edge, a, a + 3), filler, n_keys, seg, mode == V1)
                    assert reached == {"first": 2, "last": 1, "after_big": 0} and pos.tolist() == [0, 31, 32]
                    out = compare(eng, mode, arrs, n_keys, Ref(mode, arrs, n_keys), fixed=n_keys == 4, zero_hi=a % 2 == 1)
                    by_hand(out, cases[a:a + 3], pos)
                continue
            arrs, cases, pos, reached, full = batch(mode, n_keys, sh, keys, J, seg, 31 + J + n_keys)
            assert reached["first"] >= 1 and reached["after_big"] == 1
            assert reached["last"] >= 1 and full, reached    # an edge job at lane 31 / 255, at every width
            ref = Ref(mode, arrs, n_keys)
            by_hand(compare(eng, mode, arrs, n_keys, ref, fixed=n_keys == 4), cases, pos)
            by_hand(compare(eng, mode, arrs, n_keys, ref, zero_hi=True), cases, pos)


# ------------------------------------------------------------------ chunked batches

@pytest.mark.parametrize("mode", [V1, V2])
@pytest.mark.parametrize("J,zerocopy", [(8193, ""), (8193, "1"), (32768, "")])
@pytest.mark.parametrize("n_keys", [1, 4, 5, 9, 16])
def test_edges_chunked(eng, monkeypatch, n_keys, J, zerocopy, mode):
    """Above 8192 jobs the segments cross as chunks and run from HBM (PE_AGG_ZEROCOPY=1: from pinned memory):
    one host thread at 8193 jobs, the planning pool at 32768.  Every job has the containers from which a
    narrowed segment saves bytes (two; one in the small-filler stretch of the wider tables), so every
    segment of a narrowed batch is narrowed wherever it is cut, and none of an unnarrowable one: the stats
    say so.  An edge job sits at lane 0, at lane 255 of a full segment and after the oversized job; at 8193
    jobs (one job range) the engine's segment count is the restated planner's, at 32768 the batch is also
    cut at chunk and thread edges, so the lanes there are the restatement's."""
    if zerocopy:
        monkeypatch.setenv("PE_AGG_ZEROCOPY", "1")
    for sh, keys in variants(n_keys, (3,) if n_keys > 1 else (2, 7)):
        arrs, cases, pos, reached, full = batch(mode, n_keys, sh, keys, J, E.SEG_JOBS, 41 + J + n_keys, pad=2, min_cont=2)
        assert E.saves_bytes(min(E.job_sizes(arrs)[1]), E.nd_of(n_keys))
        assert reached["first"] >= 1 and reached["after_big"] == 1 and reached["last"] >= 1 and full, reached
        ref = Ref(mode, arrs, n_keys)
        eng.reset_stats()
        for a, b in zip(eng.pg_min_resources_keys(mode, *arrs), ref.o):
            np.testing.assert_array_equal(a, b)
        st = eng.stats()
        if J == 8193:
            assert st["agg_segments"] == E.planned_segments(arrs, n_keys, E.SEG_JOBS, mode == V1), st
        assert st["agg_segments"] > J // E.SEG_JOBS
        assert st["agg_narrow_segments"] == (0 if sh is None else st["agg_segments"]), (sh, st)
        by_hand(compare(eng, mode, arrs, n_keys, ref, fixed=n_keys == 4), cases, pos)


# ------------------------------------------------------------------ A/B knobs read per call

@pytest.mark.parametrize("seg_jobs", ["1", "7"])
@pytest.mark.parametrize("n_keys", [4, 5, 16])
def test_edges_segment_jobs_override(eng, monkeypatch, n_keys, seg_jobs):
    """PE_AGG_SEG_JOBS = 1 and 7: every edge job first and last of a segment, on the latency launch and
    (7) on the chunked path."""
    monkeypatch.setenv("PE_AGG_SEG_JOBS", seg_jobs)
    for mode in (V1, V2):
        for sh, keys in variants(n_keys, (6,)):
            for J in (300, 8193) if seg_jobs == "7" and n_keys == 4 else (300,):
                arrs, cases, pos, reached, full = batch(mode, n_keys, sh, keys, J, int(seg_jobs), 51 + n_keys,
                                                        with_big=False)
                assert reached["first"] >= 1 and reached["last"] >= 1 and full
                ref = Ref(mode, arrs, n_keys)
                by_hand(compare(eng, mode, arrs, n_keys, ref, fixed=n_keys == 4), cases, pos)


def test_edges_device_path(eng, monkeypatch):
    """PE_AGG_DEVICE=1 (fixed dimensions only): pg_min_resources_kernel restates agg_job_t over the caller's
    arrays in device memory -- every edge of all four dimensions, one job per call and a batch."""
    monkeypatch.setenv("PE_AGG_DEVICE", "1")
    for mode in (V1, V2):
        for sh in (None, E.key_shifts(4, 0), E.key_shifts(4, 4)):
            arrs, cases = E.edge_batch(mode, 4, sh)
            f = (*arrs[:5], E.fixed_flags(arrs[5]))
            want = oracle.pg_min_resources(mode, *f)
            np.testing.assert_array_equal(want[3], [c["flag"] for c in cases])
            for a, b in zip(eng.pg_min_resources(mode, *f), want):
                np.testing.assert_array_equal(a, b)
            for j, c in enumerate(cases):
                if c["flag"] == 0:
                    assert want[0][j, c["key"]] == c["want"], c["name"]
            for j in range(0, len(cases), 3):
                one = E.csr_slice(f, j, j + 1)
                for a, b in zip(eng.pg_min_resources(mode, *one), want):
                    np.testing.assert_array_equal(a[0], b[j])


# ------------------------------------------------------------------ an oversized edge job, read in place

@pytest.mark.parametrize("narrow", [True, False])
@pytest.mark.parametrize("n_keys", [4, 5, 16])
def test_edges_oversized_job_in_place(eng, n_keys, narrow):
    """One job of 4096 containers (more than a segment's LDS budget: read in place from pinned memory, or
    from HBM on the chunked path) whose main sum is the largest in-range value -- 2^63 - 1, or 2^63 - 2^31
    on the narrowable grid -- and exactly 2^63: alone, between ordinary jobs, and in a chunked batch."""
    for e in sorted({0, n_keys - 1}):
        sh = [31] * n_keys if narrow else None
        for out in (False, True):
            one, total = E.oversized_edge(n_keys, e, narrow, out)
            case = dict(name="oversized", key=e, want=total, flag=int(out), mem=1, pres=True)
            for mode in (V1, V2):
                for J in (1, 300, 8193) if e == n_keys - 1 else (1, 300):
                    if J == 1:
                        arrs, pos = one, np.array([0])
                    else:
                        f = E.filler_batch(J - 1, n_keys, 61 + J, sh, min_cont=2)
                        arrs = E.csr_concat([E.csr_slice(f, 0, J // 3), one, E.csr_slice(f, J // 3, J - 1)], n_keys)
                        pos = np.array([J // 3])
                    ref = Ref(mode, arrs, n_keys)
                    eng.reset_stats()
                    by_hand(compare(eng, mode, arrs, n_keys, ref, fixed=n_keys == 4, zero_hi=J == 300), [case], pos)
                    if J == 8193:                            # the keys, fixed and wide calls: three passes
                        st = eng.stats()
                        assert st["agg_narrow_segments"] == (st["agg_segments"] if narrow else 0) and st["agg_segments"]
