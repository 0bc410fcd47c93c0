#!/usr/bin/env python3
"""The domain calls under two libraries: the tree's and another build (the parent commit's, made with `make OUT=...`
from a checkout of it), in one job.

    python tools/domain_calls_ab.py OTHER_LIBRARY [tool ...]    the latency tools, each run other, tree, other
    python tools/domain_calls_ab.py --memory                    one context, every domain call once (PE_LIBRARY)

The first form runs the named latency tools (default: the six domain calls') as child processes and prints, per
row that reports a "call N us", the three medians, the spread of the other library's two runs and whether the
tree stays within the slower of them plus that spread (the kernels' own time, where the row reports it, as a row
of its own: it tells a move of the host side from one of the device side); then the second form under both
libraries.  The second form loads GC_NODES nodes (1M) in racks of GC_RACK under blocks of 32 racks, calls pe_place_greedy_domains,
pe_place_min_member_domains and pe_place_first_fit_domains at the rack level and pe_gang_fit_domains and
pe_gang_preempt_domains at the block level (segments above PL_LDS_NODES: the working copies are allocated), and
prints the device memory the five calls left allocated: the free memory torch.cuda.mem_get_info reports after the
load less the one it reports after the calls."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TOOLS = ["place_domains_latency.py", "gang_fit_latency.py", "first_fit_latency.py", "gang_preempt_latency.py",
         "place_min_member_latency.py", "drain_fit_latency.py"]
LIMIT = int(os.environ.get("AB_TOOL_LIMIT_S", "400"))


def child(args, library):
    env = dict(os.environ)
    env.pop("PE_LIBRARY", None)
    if library:
        env["PE_LIBRARY"] = library
    p = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=LIMIT)
    if p.returncode != 0:
        sys.exit(f"{args} under {library or 'the tree'} ended with {p.returncode}:\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
    return p.stdout


def rows(text):
    """{row name: call us} of a latency tool's output, and {row name + " [kernels]": kernels us} where the line has
    that too; a name that repeats gets its ordinal."""
    out = {}
    for line in text.splitlines():
        m = re.search(r"\bcall (\d+) us", line)
        if m:
            name = re.split(r"[;(]|: \d|\bcall \d", line)[0].strip(" :,")
            while name in out:
                name += "'"
            out[name] = int(m.group(1))
            k = re.search(r"\bkernels (\d+) us", line)
            if k:
                out[name + " [kernels]"] = int(k.group(1))
    return out


def memory():
    import numpy as np
    import torch

    from gang_capacity_common import NODES, ptr
    from placement import Engine, synth

    rack, jobs = int(os.environ.get("GC_RACK", "245")), int(os.environ.get("PD_JOBS", "2000"))
    inv = synth.make_inventory(NODES, synth.SEED["cfg5"], 0.2)
    b = synth.make_jobs(jobs, synth.SEED["cfg3"], "mixed")
    island = (np.arange(NODES, dtype=np.int64) // rack).astype(np.int32)
    racks = -(-(int(island.max()) + 1) // 32) * 32
    sizes = np.ascontiguousarray([racks, racks // 32], np.int32)
    parent = np.ascontiguousarray(np.arange(racks) // 32, np.int32)
    c = lambda a, t: np.ascontiguousarray(a, t)   # noqa: E731
    jgo, pri, cnt, req, need = c(b.job_group_off, np.int32), c(b.priority, np.int32), c(b.group_count, np.int32), \
        c(b.group_req, np.int64), c(b.group_need, np.uint32)
    G, P = int(jgo[-1]), int(cnt.sum())
    pods, st = np.full(max(P, 1), -1, np.int32), np.zeros(jobs, np.int32)
    dom0 = c(np.arange(jobs) % (int(island.max()) + 1), np.int32)
    dom1 = c(dom0 // 32, np.int32)
    pj = c(np.arange(jobs), np.int32)
    eng = Engine(0)
    lib, h, L = eng.lib, eng.h, len(sizes)
    eng.load_nodes(inv.cap, inv.used, inv.labels, island)
    eng.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]

    def ok(rc):
        assert rc == 0, lib.pe_last_error(h)

    ok(lib.pe_place_greedy_domains(h, jobs, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), ptr(dom0), 0, L, ptr(sizes),
                                   ptr(parent), ptr(pods), ptr(st)))
    vpods = pods.copy()                                      # the gangs it placed are the victims below
    gp, jp = np.zeros(max(G, 1), np.int32), np.zeros(jobs, np.int64)
    ok(lib.pe_place_min_member_domains(h, jobs, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), None, ptr(dom0), 0, L,
                                       ptr(sizes), ptr(parent), ptr(pods), ptr(st), ptr(gp), ptr(jp)))
    pair = np.zeros(jobs, np.int32)
    ok(lib.pe_place_first_fit_domains(h, jobs, ptr(jgo), ptr(pri), ptr(cnt), ptr(req), ptr(need), jobs, ptr(pj), ptr(dom0), 0,
                                      L, ptr(sizes), ptr(parent), ptr(pods), ptr(st), ptr(pair)))
    fits, first = np.zeros(jobs, np.uint8), np.zeros(jobs, np.int32)
    ok(lib.pe_gang_fit_domains(h, jobs, ptr(jgo), ptr(cnt), ptr(req), ptr(need), jobs, ptr(pj), ptr(dom1), 1, L, ptr(sizes),
                               ptr(parent), ptr(fits), None, None, ptr(first)))
    pvo, pv = c(np.arange(jobs + 1), np.int32), c((np.arange(jobs) + 1) % jobs, np.int32)   # one candidate victim per pair
    best = np.zeros(jobs, np.int32)
    ok(lib.pe_gang_preempt_domains(h, jobs, ptr(jgo), ptr(cnt), ptr(req), ptr(need), jobs, ptr(jgo), ptr(cnt), ptr(req),
                                   ptr(vpods), jobs, ptr(pj), ptr(dom1), ptr(pvo), ptr(pv), 1, L, ptr(sizes), ptr(parent),
                                   None, None, None, ptr(best)))
    eng.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    print(f"library: {os.environ.get('PE_LIBRARY') or 'the tree'}; {NODES} nodes, {jobs} jobs; device memory held by the "
          f"five domain calls: {(free0 - free1) / 2**20:.1f} MiB", flush=True)
    eng.close()


def main():
    other = os.path.abspath(sys.argv[1])
    tools = sys.argv[2:] or TOOLS
    print(f"{'row':<72}{'other':>9}{'tree':>9}{'other':>9}{'spread':>8}  within", flush=True)
    for tool in tools:
        runs = [rows(child([os.path.join(HERE, tool)], lib)) for lib in (other, None, other)]
        for name in runs[1]:
            if name in runs[0] and name in runs[2]:
                a, t, b = runs[0][name], runs[1][name], runs[2][name]
                print(f"{(tool[:-len('_latency.py')] + ': ' + name)[:71]:<72}{a:>9}{t:>9}{b:>9}{abs(a - b):>8}  "
                      f"{'yes' if t <= max(a, b) + abs(a - b) else 'NO'}", flush=True)
    if not sys.argv[2:]:
        for lib in (other, None):
            print(child([os.path.abspath(__file__), "--memory"], lib).strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    sys.path[:0] = [HERE]
    memory() if sys.argv[1:] == ["--memory"] else main()
