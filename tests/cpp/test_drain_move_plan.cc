// The plan of pe_drain_move_domains (csrc/pe_drain_move_plan.h): the candidates' order per active domain and the
// release bound against a brute force, and every refusal leaving the three plans as they were.  Stand-alone.
#include <stdio.h>

#include <random>

#include "pe_drain_move_plan.h"

typedef std::vector<int32_t> Vec;

static int failed = 0;
static long plans = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) printf("FAIL %s (%d)\n", name, ++failed);
}

struct Input {
  Vec off, cnt, pod, node, dom;
  std::vector<int64_t> req, res, res0;   // res, res0: [n_total][4]
  int64_t n_total;
};

static pe::DrainMoveError build(pe::DrainPlan& d, pe::DrainMovePlan& m, pe::LedgerPlan& l, const Input& in, int32_t n_dom,
                                uint32_t flags, int64_t* bad, pe::DrainPlanError* de = nullptr) {
  return pe::drain_move_plan_build(
      d, m, l, in.n_total, (int64_t)in.off.size() - 1, in.off.data(), in.cnt.data(), in.req.data(), in.pod.data(),
      (int64_t)in.node.size(), in.node.data(), in.dom.data(), 0, 1, &n_dom, nullptr, flags,
      [&](int32_t n) { return in.res[(size_t)n * 4] == pe::LEDGER_REMOVED; }, [&](int32_t n) { return &in.res[(size_t)n * 4]; },
      [&](int32_t n) { return &in.res0[(size_t)n * 4]; }, de, nullptr, nullptr, nullptr, bad);
}

// V gangs of two groups on n_total nodes (node 0 a removed slot in every third input); C distinct candidate nodes.
static Input random_input(std::mt19937& rng, int V, int C, int n_dom, int n_total, int64_t room) {
  Input in;
  in.n_total = n_total;
  in.off = {0};
  for (int g = 0; g < 2 * V; ++g) {
    in.cnt.push_back((int32_t)(rng() % 4));
    for (int d = 0; d < 4; ++d) in.req.push_back((int64_t)(rng() % 5));
    for (int s = 0; s < in.cnt.back(); ++s) in.pod.push_back((int32_t)(rng() % (n_total + 1)) - 1);
    if (g & 1) in.off.push_back(g + 1);
  }
  Vec nodes((size_t)n_total);
  std::iota(nodes.begin(), nodes.end(), 0);
  std::shuffle(nodes.begin(), nodes.end(), rng);
  in.node.assign(nodes.begin(), nodes.begin() + C);
  for (int c = 0; c < C; ++c) in.dom.push_back((int32_t)(rng() % n_dom));
  in.res.assign((size_t)n_total * 4, 100);
  in.res0.assign((size_t)n_total * 4, 100 + room);
  if (rng() % 3 == 0) in.res[0] = pe::LEDGER_REMOVED;
  return in;
}

int main() {
  std::mt19937 rng(11);
  for (int it = 0; it < 60; ++it) {
    const int n_dom = 1 + it % 4, n_total = 1 + it % 7, C = it % (n_total + 1);
    const Input in = random_input(rng, it % 6, C, n_dom, n_total, it % 2 ? 1000 : 3);
    pe::DrainPlan d;
    pe::DrainMovePlan m;
    pe::LedgerPlan l;
    int64_t bad = 99;
    const pe::DrainMoveError e = build(d, m, l, in, n_dom, (uint32_t)(it & 1), &bad);
    // ---- brute force: what every live candidate's pods give back, one pod at a time in 128 bits
    std::vector<__int128> sum((size_t)n_total * 4, 0);
    size_t s = 0;
    for (size_t g = 0; g < in.cnt.size(); ++g)
      for (int32_t k = 0; k < in.cnt[g]; ++k, ++s) {
        const int32_t n = in.pod[s];
        if (n < 0 || in.res[(size_t)n * 4] == pe::LEDGER_REMOVED || std::find(in.node.begin(), in.node.end(), n) == in.node.end())
          continue;
        for (int dd = 0; dd < 4; ++dd) sum[(size_t)n * 4 + (size_t)dd] += in.req[g * 4 + (size_t)dd];
      }
    bool crosses = false;
    for (size_t i = 0; i < sum.size(); ++i) crosses |= sum[i] > 0 && in.res[i] + sum[i] > (__int128)in.res0[i];
    check("release bound", e == (crosses ? pe::DM_OVER : pe::DM_OK));
    check("maps", l.place == Vec((size_t)n_total, -1) && d.cand_of == Vec((size_t)n_total, -1));
    if (e != pe::DM_OK) continue;
    check("built", ++plans && bad == -1 && m.dry_run == (bool)(it & 1) && d.n_cands() == C);
    // the candidates of every active domain: ascending c, each exactly once
    Vec seen((size_t)C, 0);
    for (size_t a = 0; a < d.fit.active.size(); ++a)
      for (int32_t i = d.fit.pair_start[a]; i < d.fit.pair_start[a + 1]; ++i) {
        const int32_t c = d.fit.pairs[(size_t)i];
        check("domain", in.dom[(size_t)c] == d.fit.active[a]);
        check("ascending", i == d.fit.pair_start[a] || d.fit.pairs[(size_t)i - 1] < c);
        ++seen[(size_t)c];
      }
    check("each once", seen == Vec((size_t)C, 1));
  }
  // ---- refusals, in the order of the checks; the three plans stay as they were
  Input good;
  good.n_total = 3;
  good.off = {0, 1, 2}, good.cnt = {1, 2}, good.req = {1, 0, 0, 0, 2, 0, 0, 0}, good.pod = {0, 1, 1};
  good.node = {1, 0}, good.dom = {1, 0};
  good.res = {5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5}, good.res0 = {6, 5, 5, 5, 9, 5, 5, 5, 5, 5, 5, 5};
  pe::DrainPlan d;
  pe::DrainMovePlan m;
  pe::LedgerPlan l;
  int64_t bad = 99;
  check("a plan to keep", build(d, m, l, good, 2, 1, &bad) == pe::DM_OK && d.slot_list == Vec({1, 2, 0}) && l.pods == 3);
  const pe::LedgerPlan l0 = l;
  auto refused = [&](const char* name, Input in, uint32_t flags, pe::DrainMoveError want, int64_t want_index,
                     pe::DrainPlanError want_drain = pe::DRAIN_OK) {
    pe::DrainPlanError de = pe::DRAIN_OK;
    const pe::DrainMoveError e = build(d, m, l, in, 2, flags, &bad, &de);
    check(name, e == want && bad == want_index && de == want_drain && d.slot_list == Vec({1, 2, 0}) && d.n_runs() == 2 &&
                    d.cand_of == Vec(3, -1) && d.fit.pairs == Vec({1, 0}) && m.dry_run && l.place == l0.place &&
                    l.pods == 3 && l.touched.size() == 2);
    ++refusals;
  };
  Input in = good;
  in.pod = {0, 1, 3}, refused("pod_node", in, 2, pe::DM_BAD_DRAIN, 2, pe::DRAIN_BAD_GANGS);
  in = good, in.node = {1, 1}, refused("repeated cand_node", in, 2, pe::DM_BAD_DRAIN, 1, pe::DRAIN_DUP_NODE);
  in = good, in.dom = {1, 2}, refused("cand_domain", in, 2, pe::DM_BAD_DRAIN, 1, pe::DRAIN_BAD_FIT);
  refused("flags", good, 2, pe::DM_BAD_FLAGS, -1);
  in = good, in.req[4] = 3, refused("release bound", in, 0, pe::DM_OVER, 1);
  in = good, in.req[4] = INT64_MAX, refused("release bound in 128 bits", in, 0, pe::DM_OVER, 1);
  printf("%ld plans, %ld refusals, %d failures\n", plans, refusals, failed);
  return failed ? 1 : 0;
}
