// The plan of pe_place_preempt_domains (training-operator_amd/csrc/pe_place_preempt_plan.h): the victims' owner
// domains, the release records and the jobs' list ranges against a brute force on random inputs, and every refusal,
// each leaving the plan and the ledger scratch as they were.  Stand-alone; tests/test_place_preempt_plan_cpu.py
// builds and runs it.
#include <stdio.h>

#include <random>

#include "pe_place_preempt_plan.h"

using pe::PlacePreemptPlan;
typedef std::vector<int32_t> Vec;

static int failed = 0;
static long plans = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

struct Input {
  Vec off, pri, cnt, dom, voff, vcnt, vpod, jvo, jv;
  std::vector<int64_t> vreq;
  int64_t n_total;
  std::vector<int64_t> res, res0;   // [n_total][4]
};

static pe::PlacePreemptError build(PlacePreemptPlan& p, pe::LedgerPlan& l, const Input& in, int32_t n_dom, uint32_t flags,
                                   int64_t* bad, pe::PreemptPlanError* ve = nullptr) {
  return pe::place_preempt_plan_build(
      p, l, (int64_t)in.pri.size(), in.off.data(), in.pri.data(), in.cnt.data(), in.dom.data(), 0, 1, &n_dom, nullptr,
      in.n_total, (int64_t)in.voff.size() - 1, in.voff.data(), in.vcnt.data(), in.vreq.data(), in.vpod.data(),
      in.jvo.data(), in.jv.data(), flags, [&](int32_t n) { return &in.res[(size_t)n * 4]; },
      [&](int32_t n) { return &in.res0[(size_t)n * 4]; }, nullptr, nullptr, ve, bad);
}

// J jobs of one group over n_dom domains, V victims of two groups; every domain's jobs list that domain's victims
// (victim v belongs to domain v % n_dom), each list a random subset in random order.
static Input random_input(std::mt19937& rng, int J, int V, int n_dom, int n_total) {
  Input in;
  in.n_total = n_total;
  in.off = in.jvo = in.voff = {0};
  for (int v = 0; v < V; ++v) {
    for (int g = 0; g < 2; ++g) {
      in.vcnt.push_back((int32_t)(rng() % 4));
      for (int d = 0; d < 4; ++d) in.vreq.push_back((int64_t)(rng() % 5));
      for (int s = 0; s < in.vcnt.back(); ++s) in.vpod.push_back((int32_t)(rng() % (n_total + 1)) - 1);
    }
    in.voff.push_back((int32_t)in.vcnt.size());
  }
  for (int j = 0; j < J; ++j) {
    in.pri.push_back((int32_t)(rng() % 3));
    in.cnt.push_back((int32_t)(rng() % 3));
    in.off.push_back(j + 1);
    in.dom.push_back((int32_t)(rng() % n_dom));
    Vec mine;
    for (int v = in.dom.back(); v < V; v += n_dom)
      if (rng() % 2) mine.push_back(v);
    std::shuffle(mine.begin(), mine.end(), rng);
    in.jv.insert(in.jv.end(), mine.begin(), mine.end());
    in.jvo.push_back((int32_t)in.jv.size());
  }
  in.res.assign((size_t)n_total * 4, 100);
  in.res0.assign((size_t)n_total * 4, 100 + 4 * 3 * 2 * (int64_t)V);   // room for every victim on one node
  return in;
}

int main() {
  std::mt19937 rng(7);
  for (int it = 0; it < 40; ++it) {
    const int n_dom = 1 + it % 4, V = it % 9, n_total = 1 + it % 6;
    const Input in = random_input(rng, 1 + it % 7, V, n_dom, n_total);
    PlacePreemptPlan p;
    pe::LedgerPlan l;
    int64_t bad = 99;
    check("built", build(p, l, in, n_dom, (uint32_t)(it & 1), &bad) == pe::PP_OK && bad == -1 && p.dry_run == (it & 1));
    ++plans;
    // ---- brute force: owners from the lists, one record per run of one node in a group, the jobs' ranges
    for (int v = 0; v < V; ++v) {
      int32_t owner = -1;
      for (size_t j = 0; j < in.dom.size(); ++j)
        for (int32_t i = in.jvo[j]; i < in.jvo[j + 1]; ++i)
          if (in.jv[(size_t)i] == v) owner = in.dom[j];
      check("owner", p.vic_owner[(size_t)v] == owner && p.vic_act[(size_t)v] == (owner < 0 ? -1 : p.base.act_of[(size_t)owner]));
    }
    std::vector<pe::PreRec> want;   // one pod at a time: a record begins where the node changes or the group does
    size_t s = 0;
    for (int v = 0; v < V; ++v) {
      check("rec_start", p.rec_start[(size_t)v] == (int32_t)want.size());
      for (int32_t g = in.voff[(size_t)v]; g < in.voff[(size_t)v + 1]; ++g)
        for (int32_t c = 0; c < in.vcnt[(size_t)g]; ++c, ++s) {
          if (in.vpod[s] < 0) continue;
          if (c == 0 || in.vpod[s - 1] != in.vpod[s]) want.push_back(pe::PreRec{{0, 0, 0, 0}, in.vpod[s], 0});
          for (int d = 0; d < 4; ++d) want.back().q[d] += in.vreq[(size_t)g * 4 + (size_t)d];
        }
    }
    check("records", want.size() == p.recs.size() && p.rec_start[(size_t)V] == (int32_t)want.size());
    for (size_t r = 0; r < want.size() && r < p.recs.size(); ++r)
      check("record", want[r].node == p.recs[r].node && std::equal(want[r].q, want[r].q + 4, p.recs[r].q));
    for (size_t i = 0; i < p.jobs.size(); ++i) {
      const pe::PreemptJob& pj = p.jobs[i];
      check("job", pj.job == p.base.jobs[i] && pj.g0 == in.off[(size_t)pj.job] && pj.g1 == in.off[(size_t)pj.job + 1] &&
                       pj.v0 == in.jvo[(size_t)pj.job] && pj.v1 == in.jvo[(size_t)pj.job + 1]);
    }
    check("ledger", l.place == Vec((size_t)n_total, -1));
  }
  // ---- refusals, in the order of the checks; the plan and the ledger scratch stay as they were
  Input good;
  good.n_total = 2;
  good.off = {0, 1, 2}, good.pri = {0, 1}, good.cnt = {1, 1}, good.dom = {0, 1};
  good.voff = {0, 1, 2}, good.vcnt = {1, 1}, good.vreq = {1, 0, 0, 0, 2, 0, 0, 0}, good.vpod = {0, 1};
  good.jvo = {0, 1, 2}, good.jv = {0, 1};
  good.res = {5, 5, 5, 5, 5, 5, 5, 5}, good.res0 = {6, 5, 5, 5, 7, 5, 5, 5};
  PlacePreemptPlan p;
  pe::LedgerPlan l;
  int64_t bad = 99;
  check("a plan to keep", build(p, l, good, 2, 0, &bad) == pe::PP_OK && p.vic_owner == Vec({0, 1}) && l.pods == 2);
  const pe::LedgerPlan l0 = l;
  auto refused = [&](const char* name, Input in, uint32_t flags, pe::PlacePreemptError want, int64_t want_index,
                     pe::PreemptPlanError want_pre = pe::PRE_OK) {
    pe::PreemptPlanError ve = pe::PRE_OK;
    const pe::PlacePreemptError e = build(p, l, in, 2, flags, &bad, &ve);
    check(name, e == want && bad == want_index && ve == want_pre && p.vic_owner == Vec({0, 1}) && p.jobs.size() == 2 &&
                    p.recs.size() == 2 && !p.dry_run && l.place == l0.place && l.pods == l0.pods && l.touched.size() == 2);
    ++refusals;
  };
  Input in = good;
  in.dom = {0, 2}, refused("job_domain", in, 2, pe::PP_BAD_PLACE, 1);
  in = good, in.vpod = {0, 2}, refused("vic_pod_node", in, 2, pe::PP_BAD_VICTIMS, 1, pe::PRE_BAD_POD_NODE);
  in = good, in.jv = {0, 2}, refused("list range", in, 2, pe::PP_BAD_VICTIMS, 1, pe::PRE_BAD_LIST_VICTIM);
  in = good, in.jvo = {0, 2, 2}, in.jv = {1, 1}, refused("duplicate", in, 2, pe::PP_BAD_VICTIMS, 1, pe::PRE_DUP_VICTIM);
  in = good, in.jvo = {0, 66, 66}, in.jv = Vec(66, 0), refused("list of 66", in, 2, pe::PP_BAD_VICTIMS, 0, pe::PRE_LONG_LIST);
  in = good, in.jv = {0, 0}, refused("two domains", in, 2, pe::PP_TWO_DOMAINS, 1);
  refused("flags", good, 2, pe::PP_BAD_FLAGS, -1);
  in = good, in.vreq[4] = 3, refused("release bound", in, 0, pe::PP_OVER, 1);
  in = good, in.vreq[0] = INT64_MAX, in.vcnt[0] = 2, in.vpod = {0, 0, 1}, refused("release bound in 128 bits", in, 0, pe::PP_OVER, 0);
  printf("%ld plans, %ld refusals, %d failures\n", plans, refusals, failed);
  return failed ? 1 : 0;
}
