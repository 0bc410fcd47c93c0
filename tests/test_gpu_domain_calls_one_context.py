"""The five domain calls on ONE context.  They share one host path and one set of buffers (pe_domain_call.h, pe_ctx.h
dm_*), so what could go wrong is a call seeing an earlier call's content: a buffer larger than the call needs that
still holds the previous calls' bytes beyond its span, large-segment records and working copies left by a call
with another number of units, a stride that shrank while the buffers kept their size.  One engine walks through the
calls on two inventories; every answer is compared with its CPU checker and with the same call made alone on a
fresh engine loaded with the same residuals, and the residuals with the checker's after every placing call and with
what they were after every read-only one."""
import numpy as np
import pytest

import domain_capacity as DC
import domain_placement as DP
import first_fit as FF
import gang_fit as GF
import gang_preempt as GP
import min_member as MM
from placement import Engine, synth

pytestmark = pytest.mark.gpu

LDS = 1016                           # pe_kernels.h PL_LDS_NODES
GiB = 1 << 30


class Inventory:
    def __init__(self, cap, used, labels, island, level_size, parent, vic=None, held=None):
        self.cap, self.used, self.labels, self.island = cap, used, labels, island
        self.level_size, self.parent, self.vic, self.held = level_size, parent, vic, held or {}


def inventory_s():
    """96 nodes in racks of 8: 12 racks -> 3 blocks -> 1 root."""
    island = np.arange(96, dtype=np.int32) // 8
    parent = np.concatenate([np.arange(12) // 4, np.zeros(3)]).astype(np.int32)
    return Inventory(*DC.with_islands(synth.make_inventory(96, 23), island), [12, 3, 1], parent)


def inventory_l():
    """1100 nodes, one level: a rack of 1040 nodes (above PL_LDS_NODES) beside three racks of 20, dealt in a shuffled
    order, with resident gangs (gang_preempt.resident_victims) accounted in `used`: the victims of the walk's step 9."""
    jobs = [(0, p, [(3, [2000, 4 * GiB, 0, 0], 0), (2, [500, GiB, 1, 0], 1)]) for p in range(4)] + \
           [(0, 2, [(2, [8000, 16 * GiB, 0, 0], DP.ISLAND)]), (1, 1, [(1, [500, GiB, 0, 0], 0)])]
    base = DP.one_level_case([1040, 20, 20, 20], jobs, seed=43, pad=0)
    assert len(base.island) == 1100 and np.bincount(base.island).tolist() == [1040, 20, 20, 20] and 1040 > LDS
    vic, res, held = GP.resident_victims(base, rounds=2, want=6)
    return Inventory(base.cap, base.cap - res, base.labels, base.island, [4], None, vic, held)


def few(batch, dom, k, n, mm=None):
    """The mix cut to a handful: the jobs of the first k distinct domains it names, one job of each at least, n in
    all where it has them; the min_member values go with their jobs."""
    doms = list(dict.fromkeys(int(d) for d in dom))[:k]
    assert len(doms) == k
    first = [int(np.nonzero(dom == d)[0][0]) for d in doms]
    rest = [j for j in range(len(dom)) if int(dom[j]) in doms and j not in first]
    keep = sorted(first + rest[:max(0, n - k)])
    b, d = DP.make_batch([(int(dom[j]), int(batch.priority[j]), GF.job_groups(batch, j)) for j in keep])
    assert len(np.unique(d)) == k
    return (b, d) if mm is None else (b, d, np.asarray(mm, dtype=np.int32)[keep])


def same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (i, np.asarray(g).tolist()[:20], np.asarray(w).tolist()[:20])


class Walk:
    """The engine under test beside what it holds: the inventory, and the gangs its own placing calls put there."""

    def __init__(self, eng, fresh):
        self.eng, self.fresh, self.seed, self.placed, self.evictions, self.refusals = eng, fresh, 500, 0, 0, 0

    def load(self, inv):
        self.inv, self.gangs = inv, []
        self.eng.load_nodes(inv.cap, inv.used, inv.labels, inv.island)

    def case(self, res, level, batch, dom):
        v = self.inv
        return DP.Case(v.cap, v.cap - res, v.labels, v.island, list(v.level_size), v.parent, level, batch, dom)

    def mix(self, res, level, k, n, module=DP):
        self.seed += 1
        v = self.inv
        out = module.job_mix(res, v.labels, v.island, level, v.level_size, v.parent, self.seed, max_domains=k)
        return few(out[0], out[1], k, n, *out[2:])

    def run(self, res, call, want, want_res):
        """The call on the engine under test and alone on a fresh engine at the same residuals: both as the checker
        says, and the residuals afterwards too."""
        v = self.inv
        got = tuple(call(self.eng))
        same(got, want)
        assert np.array_equal(self.eng.read_residuals(), want_res)
        alone = self.fresh()
        alone.load_nodes(v.cap, v.cap - res, v.labels, v.island)
        same(tuple(call(alone)), got)
        assert np.array_equal(alone.read_residuals(), want_res)
        alone.close()
        return got

    def took(self, batch, pods, status):
        """The placed jobs that hold a pod join the resident gangs: priority, and per group the request and the slots."""
        poff = DP.pod_offsets(batch.group_count)
        for j in np.nonzero(np.asarray(status) == 0)[0]:
            g0, g1 = int(batch.job_group_off[j]), int(batch.job_group_off[j + 1])
            groups = [([int(x) for x in batch.group_req[g]], [int(x) for x in pods[poff[g]:poff[g + 1]]]) for g in range(g0, g1)]
            if any(n >= 0 for _, nodes in groups for n in nodes):
                self.gangs.append((int(batch.priority[j]), groups))
                self.placed += 1

    # ---- the five calls; `domains`: how many domains of `level` are active

    def fit(self, level, domains, per_domain=1):
        """Every active domain paired with the jobs in turn, the first of them per_domain times over (a domain's pairs
        are cut into units of 32), in a shuffled order."""
        res = self.eng.read_residuals()
        v = self.inv
        batch, dom = self.mix(res, level, 1, 4)
        jobs = [(0, 0, GF.job_groups(batch, j)) for j in range(len(dom))]
        jobs += [(0, 0, [(1, [1, 0, 0, 0], DP.NO_LABEL)]), (0, 0, [(2, [500, GiB, 0, 0], 0), (1, [10**9, 0, 0, 0], 0)])]
        batch, _ = DP.make_batch(jobs)                       # ... and two jobs that fit nowhere: fail_group 0 and 1
        J = len(batch.priority)
        active = np.random.default_rng(self.seed).permutation(int(v.level_size[level]))[:domains]
        if v.vic is not None:
            active = np.concatenate([[0], active[active != 0][:domains - 1]])      # the large rack among them
        pd = np.concatenate([np.repeat(active[:1], per_domain * J), active[1:]]).astype(np.int32)
        pj = (np.arange(len(pd)) % J).astype(np.int32)
        order = np.random.default_rng(self.seed).permutation(len(pd))
        pj, pd = pj[order], pd[order]
        assert len(np.unique(pd)) == domains
        fits, fail, pods = GF.answers(res, v.labels, v.island, batch, pj, pd, level, v.level_size, v.parent)
        want = (fits, fail, pods, GF.first_of(pj, fits, J))

        def call(e):
            got = e.gang_fit_domains(batch.job_group_off, batch.group_count, batch.group_req, batch.group_need, pj, pd,
                                     level, v.level_size, v.parent)
            return got.fits, got.fail_group, got.pods, got.first
        self.refusals += int((fits == 0).sum())
        return self.run(res, call, want, res)

    def preempt(self, level, vic, held, domain, per_job):
        """A handful of incoming jobs -- the first and the last of gang_preempt.incoming_mix, where the jobs that need
        an eviction are, and one pod more of a resident pod's cpu than `domain` holds until that resident is gone --
        each paired per_job times with `domain` (a domain's pairs are cut into units of 4) and once with another one;
        gang_preempt.pair_lists' candidate lists."""
        res = self.eng.read_residuals()
        v = self.inv
        self.seed += 1
        c0 = self.case(res, level, *DP.make_batch([]))
        batch, dom = GP.incoming_mix(res, c0, vic, held, self.seed)
        d_of = DP.dom_level(v.island, level, v.level_size, v.parent)
        usable = (d_of == domain) & (res >= 0).all(axis=0)
        x = max(q[0] for g in range(len(vic)) for n, q in vic.pods(g) if usable[n])      # a resident pod's cpu there
        needy = (int((res[0][usable] // x).sum()) + 1, [x, 0, 0, 0], 0)
        jobs = [(int(dom[j]), int(batch.priority[j]), GF.job_groups(batch, j)) for j in (0, 1, 2, len(dom) - 2, len(dom) - 1)]
        batch, dom = DP.make_batch(jobs + [(domain, 50, [needy])])
        J = len(dom)
        other = (domain + 1) % int(v.level_size[level])
        pj = np.concatenate([np.repeat(np.arange(J), per_job), np.arange(J) if domain != other else []]).astype(np.int32)
        pd = np.concatenate([np.full(J * per_job, domain), np.full(len(pj) - J * per_job, other)]).astype(np.int32)
        case = self.case(res, level, batch, dom)
        pvo, pv = GP.pair_lists(case, vic, pj, pd, self.seed)
        pc = GP.PCase(case, vic, pj, pd, pvo, pv)
        got = self.run(res, lambda e: tuple(e.gang_preempt_domains(*pc.call_args())), pc.answers(res), res)
        self.evictions += int((np.asarray(got[2]) > 0).sum())

    def greedy(self, level, domains):
        res = self.eng.read_residuals()
        v = self.inv
        batch, dom = self.mix(res, level, domains, 8)
        want = DP.place(res, v.labels, v.island, batch, dom, level, v.level_size, v.parent)
        pods, st = self.run(res, lambda e: e.place_greedy_domains(batch.job_group_off, batch.priority, batch.group_count,
                                                                  batch.group_req, batch.group_need, dom, level, v.level_size,
                                                                  v.parent), want[:2], want[2])
        self.took(batch, pods, st)

    def min_member(self, level, domains):
        res = self.eng.read_residuals()
        v = self.inv
        batch, dom, mm = self.mix(res, level, domains, 8, MM)
        want = MM.place(res, v.labels, v.island, batch, mm, dom, level, v.level_size, v.parent)
        jgo = [int(x) for x in batch.job_group_off]
        job_pods = np.array([int(want[2][g0:g1].sum()) for g0, g1 in zip(jgo, jgo[1:])], dtype=np.int64)
        pods, st, _, _ = self.run(res, lambda e: e.place_min_member_domains(
            batch.job_group_off, batch.priority, batch.group_count, batch.group_req, batch.group_need, mm, dom, level,
            v.level_size, v.parent), want[:3] + (job_pods,), want[3])
        self.took(batch, pods, st)

    def first_fit(self, level, domains):
        res = self.eng.read_residuals()
        v = self.inv
        batch, dom = self.mix(res, level, min(domains, int(v.level_size[level])), 6)
        case, pj, pd = FF.pair_lists(self.case(res, level, batch, dom), self.seed, res)
        chosen = list(dict.fromkeys(int(d) for d in pd))[:domains]
        keep = np.isin(pd, chosen)
        pj, pd, batch = pj[keep], pd[keep], case.batch
        assert len(np.unique(pd)) == min(domains, int(v.level_size[level]))
        want = FF.place_first_fit(res, v.labels, v.island, batch, pj, pd, level, v.level_size, v.parent)
        pods, st, _ = self.run(res, lambda e: e.place_first_fit_domains(batch.job_group_off, batch.priority, batch.group_count,
                                                                        batch.group_req, batch.group_need, pj, pd, level,
                                                                        v.level_size, v.parent), want[:3], want[3])
        self.took(batch, pods, st)

    def victims(self):
        assert self.gangs, "the placing calls before this one placed nothing"
        return GP.make_victims(self.gangs)

    def busiest(self, level, vic):
        """The domain of `level` in which the resident gangs hold the most pods."""
        v = self.inv
        dom = DP.dom_level(v.island, level, v.level_size, v.parent)
        nodes = [n for g in range(len(vic)) for n, _ in vic.pods(g)]
        return int(np.bincount(dom[nodes]).argmax())


def walk(eng, fresh, S, L):
    w = Walk(eng, fresh)

    def steps_1_to_3():
        w.fit(0, 12)                                         # 1: every rack active
        w.greedy(1, 2)                                       # 2: two blocks
        vic = w.victims()
        w.preempt(0, vic, {}, w.busiest(0, vic), 2)          # 3: one rack contested (and its neighbour once per job)

    w.load(S)
    steps_1_to_3()
    w.first_fit(0, 5)                                        # 4: five racks
    w.min_member(1, 3)                                       # 5: three blocks
    w.fit(0, 1)                                              # 6: one rack: every buffer larger than the call needs
    w.load(L)                                                # 7
    w.fit(0, 2, per_domain=7)                                # 8: 42 pairs on the large rack (2 units) and a small rack
    w.preempt(0, L.vic, L.held, 0, 2)                        # 9: 12 pairs on the large rack (3 units) and a small rack
    w.fit(0, 2)                                              # 10: 6 pairs on the large rack (1 unit)
    w.first_fit(0, 4)                                        # 11
    w.greedy(0, 4)                                           # 12
    w.load(S)                                                # 13: the stride shrinks, the buffers keep L's size
    steps_1_to_3()                                           # 14
    return w.placed, w.evictions, w.refusals


def test_the_five_calls_on_one_context():
    eng = Engine(0)
    placed, evictions, refusals = walk(eng, lambda: Engine(0), inventory_s(), inventory_l())
    eng.close()
    assert placed >= 4 and evictions >= 3 and refusals >= 6  # gangs placed, pairs that need an eviction, pairs that do not fit
