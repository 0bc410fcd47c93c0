"""The sharded greedy across PROCESSES on the GPU box: 2 (and 3) separate rank processes, each with its
own engine context holding one node shard on device 0, exchanging candidate blobs over gloo through
the pe_config.exchange hook.  Every rank must return the unsharded oracle's placements, and the
concatenated shard residuals must equal the oracle's -- for two consecutive batches (the second on
the inventory the first left).  This is the cross-process protocol of the multi-GPU runs, with gloo
standing in for RCCL on a one-GPU box."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle
from host_register import REASON as HOST_REGISTER_REASON
from host_register import host_register_supported
from placement import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(tmp_path, world, mix, n_nodes, n_jobs, transport, env):
    port = free_port()
    return [subprocess.Popen([sys.executable, os.path.join(HERE, "mp_shard_worker.py"), str(r), str(world), str(port),
                              mix, str(n_nodes), str(n_jobs), str(tmp_path), transport], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]


def _env(**kv):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PE_HOST_MERGE", "PE_NO_ZC_EXCHANGE", "PE_HX_GPU_TIMEOUT_S", "PE_MERGE_RANKED",
              "PE_MERGE_SORT", "PE_ZC_DEV_MERGE", "PE_HX_TIMEOUT_S", "PE_XCHG_THREADS"):
        env.pop(k, None)
    env.update(kv)
    return env


@pytest.mark.parametrize("world,mix,n_nodes,n_jobs,host_merge,transport", [(2, "mixed", 20000, 600, False, "gloo"),
                                                                           (3, "gang8", 9000, 300, False, "gloo"),
                                                                           (2, "island8", 6000, 300, True, "gloo"),
                                                                           (2, "mixed", 20000, 600, False, "shm"),
                                                                           (3, "island8", 9000, 300, False, "shm"),
                                                                           (2, "mixed", 20000, 600, False, "shm-copy"),
                                                                           (3, "mixed", 2, 40, False, "shm"),
                                                                           (2, "mixed", 20000, 600, False, "shm-sortmerge"),
                                                                           (2, "mixed", 20000, 600, False, "shm-devmerge"),
                                                                           (3, "gang8", 9000, 300, False, "shm-devmerge"),
                                                                           (3, "island8", 9000, 300, False, "gloo-ranked"),
                                                                           (2, "gang8", 6000, 300, True, "shm"),
                                                                           (2, "gang8", 6000, 300, False, "shm-grow"),
                                                                           (3, "island8", 9000, 300, False, "shm-grow"),
                                                                           # five ranks, the host merge on 3 threads
                                                                           # (groups split unevenly, w mod 3)
                                                                           (5, "mixed", 25000, 400, False, "shm-t3"),
                                                                           # eight ranks: BASELINE cfg3's split
                                                                           (8, "mixed", 40000, 600, False, "shm"),
                                                                           (8, "island8", 16000, 300, False,
                                                                            "shm-devmerge"),
                                                                           (8, "mixed", 40000, 600, False, "shm-copy")])
def test_sharded_greedy_across_processes(tmp_path, world, mix, n_nodes, n_jobs, host_merge, transport):
    """host_merge False: the gathered shard lists are merged on the device (the default: the rank
    merge at 2 ranks, the top-K sort merge from 3); True: PE_HOST_MERGE=1, the host's lazy k-way
    merge.  transport: the Python gloo callback, or the native shared-memory exchange
    (pe_host_exchange) -- "shm": its zero-copy windows (walk into the registered segment, the
    exchange thread merges each group on the host as every rank signalled it), "shm-devmerge":
    zero-copy with the device wait + merge kernel (PE_ZC_DEV_MERGE=1), "shm-copy": the copying
    all-gather (PE_NO_ZC_EXCHANGE=1); "-sortmerge" / "-ranked": the other merge kernel forced
    (PE_MERGE_SORT=1 at 2 ranks, PE_MERGE_RANKED=1 at 3); "shm-grow": zero-copy with lists of 8 keys
    that rescan and segment slots for the grown stride (the ranks' lists grow after the first
    rescan); "shm-t3": zero-copy with the host merge shared by 3 threads (PE_XCHG_THREADS).  Either way
    the windows are pipelined.  (3 ranks over 2 nodes: one rank's shard is
    empty -- its windows are empty lists, signalled.)"""
    base, _, variant = transport.partition("-")
    extra = {"copy": {"PE_NO_ZC_EXCHANGE": "1"}, "sortmerge": {"PE_MERGE_SORT": "1"}, "ranked": {"PE_MERGE_RANKED": "1"},
             "devmerge": {"PE_ZC_DEV_MERGE": "1"}, "grow": {}, "t3": {"PE_XCHG_THREADS": "3"}, "": {}}[variant]
    env = _env(**({"PE_HOST_MERGE": "1"} if host_merge else {}), **extra)
    zc_expected = base == "shm" and variant != "copy" and not host_merge
    if zc_expected and not host_register_supported():
        pytest.skip(HOST_REGISTER_REASON)
    transport = "shm-grow" if variant == "grow" else base
    procs = _spawn(tmp_path, world, mix, n_nodes, n_jobs, transport, env)
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=100 if world <= 3 else 200)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"
        if os.environ.get("PE_GREEDY_TRACE"):   # (diagnostics: each rank's window trace, with pytest -s)
            print(f"--- rank {r}\n{outs[r][-3000:]}")
    inv = synth.make_inventory(n_nodes, 3, 0.2 if mix != "gang8" else 1.0)
    batch = synth.make_jobs(n_jobs, 3, mix)
    w_pods, w_st, w_res = oracle.place_greedy(inv.residual(), inv.labels, batch.job_group_off, batch.priority,
                                              batch.group_count, batch.group_req, batch.group_need)
    batch2 = synth.make_jobs(n_jobs // 2, 4, mix)
    w_pods2, w_st2, w_res2 = oracle.place_greedy(w_res, inv.labels, batch2.job_group_off, batch2.priority,
                                                 batch2.group_count, batch2.group_req, batch2.group_need)
    full, full2 = np.zeros_like(w_res), np.zeros_like(w_res2)
    covered = 0
    for r in range(world):
        d = np.load(tmp_path / f"rank{r}.npz")
        np.testing.assert_array_equal(d["st"], w_st)
        np.testing.assert_array_equal(d["pods"], w_pods)
        np.testing.assert_array_equal(d["st2"], w_st2)
        np.testing.assert_array_equal(d["pods2"], w_pods2)
        b, e = int(d["b"]), int(d["e"])
        full[:, b:e] = d["res"]
        full2[:, b:e] = d["res2"]
        covered += e - b
        assert int(d["windows"]) > 1
        assert (int(d["zc"]) > 0) == zc_expected, (r, int(d["zc"]))
        if variant == "grow":
            assert int(d["rescans"]) > 0   # the short lists did run out
    assert covered == n_nodes
    np.testing.assert_array_equal(full, w_res)
    np.testing.assert_array_equal(full2, w_res2)
    assert 0 < (w_st == 0).sum() <= n_jobs
    if world == 8 and transport == "shm" and zc_expected:
        # verdict r5 item 3: at 8 ranks the exchange's host merge (the exchange thread + 3 helpers, groups
        # shared among them) keeps up with the resolve -- per window, each rank's merge time against its
        # own resolve time, over both batches (the 8 ranks share this box's one GPU and its CPUs)
        for r in range(world):
            d = np.load(tmp_path / f"rank{r}.npz")
            merge, host = float(d["xmerge_ms"]), float(d["host_ms"])
            print(f"rank {r}: exchange merge {merge:.3f} ms, wait {float(d['xwait_ms']):.3f} ms, "
                  f"resolve {host:.3f} ms over {int(d['windows'])} windows")
            assert merge <= host, (r, merge, host, int(d["windows"]))


@pytest.mark.parametrize("dev_merge", [False, True])
def test_zero_copy_exchange_peer_stall_fails_fast(tmp_path, dev_merge):
    """A rank that stops taking part (it sleeps, then exits) must not hang its peers: the exchange
    thread's wait for its lists gives up after PE_HX_TIMEOUT_S (PE_ZC_DEV_MERGE=1: the device wait
    after PE_HX_GPU_TIMEOUT_S) and the greedy call fails with PE_ERCCL."""
    if not host_register_supported():
        pytest.skip(HOST_REGISTER_REASON)
    env = _env(PE_HX_GPU_TIMEOUT_S="3", PE_HX_TIMEOUT_S="3", **({"PE_ZC_DEV_MERGE": "1"} if dev_merge else {}))
    procs = _spawn(tmp_path, 2, "mixed", 20000, 600, "shm-stall", env)
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=100)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"
        if os.environ.get("PE_GREEDY_TRACE"):   # (diagnostics: each rank's window trace, with pytest -s)
            print(f"--- rank {r}\n{outs[r][-3000:]}")
    d = np.load(tmp_path / "stall.npz")
    assert int(d["zc0"]) > 0                      # the first batch ran zero-copy on both ranks
    err = str(d["err"])
    assert err.startswith("-5:"), err              # PE_ERCCL
    assert "never arrived" in err, err
    assert float(d["secs"]) < 30, float(d["secs"])
