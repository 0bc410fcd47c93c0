// The plan of pe_place_best_fit_domains (training-operator_amd/csrc/pe_best_fit_plan.h): random pair lists against a
// brute force -- the repeats, the kept pairs, every domain's queue in rank order, the reference groups -- and every
// refusal, each leaving the plan as it was.  Stand-alone; tests/test_best_fit_plan_cpu.py builds and runs it.
#include <stdio.h>

#include <random>
#include <set>

#include "pe_best_fit_plan.h"

using pe::BestFitPlan;
typedef std::vector<int32_t> Vec;
static int failed = 0;
static long plans = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) failed += printf("FAIL %s\n", name) > 0;
}

// One level of n_dom domains; J jobs with up to three groups, P pairs drawn with many repeats and equal priorities.
static void verify(unsigned seed, int32_t J, int32_t n_dom, int32_t P) {
  std::mt19937 rng(seed);
  auto below = [&](int32_t n) { return (int32_t)(rng() % (uint32_t)n); };
  Vec off = {0}, pri, cnt, pj, pd;
  for (int32_t j = 0; j < J; ++j) {
    for (int32_t g = below(4); g > 0; --g) cnt.push_back(below(3) == 0 ? 0 : below(4));
    off.push_back((int32_t)cnt.size());
    pri.push_back(below(3));
  }
  for (int32_t p = 0; p < P; ++p) pj.push_back(below(J)), pd.push_back(below(n_dom));
  BestFitPlan pl;
  check("build", pe::best_fit_plan_build(pl, J, off.data(), pri.data(), cnt.data(), P, pj.data(), pd.data(), 0, 1, &n_dom,
                                         nullptr) == pe::FIT_OK);
  ++plans;
  // brute force: a pair is a repeat iff a smaller pair has its job and its domain
  size_t kept = 0;
  for (int32_t p = 0; p < P; ++p) {
    bool rep = false;
    for (int32_t q = 0; q < p; ++q) rep |= pj[(size_t)q] == pj[(size_t)p] && pd[(size_t)q] == pd[(size_t)p];
    check("repeat", pl.repeat[(size_t)p] == (rep ? 1 : 0));
    kept += !rep;
  }
  check("kept total", pl.kept.size() == kept && pl.queue.size() == kept && pl.kept_start.size() == (size_t)J + 1);
  for (int32_t j = 0; j < J; ++j) {
    const int32_t k0 = pl.kept_start[(size_t)j], k1 = pl.kept_start[(size_t)j + 1];
    for (int32_t k = k0; k < k1; ++k)
      check("kept order", pj[(size_t)pl.kept[(size_t)k]] == j && !pl.repeat[(size_t)pl.kept[(size_t)k]] &&
                              (k == k0 || pl.kept[(size_t)k - 1] < pl.kept[(size_t)k]));
    int32_t ref = -1, most = 0;   // the largest count, ties to the first; no pods: none
    for (int32_t g = off[(size_t)j]; g < off[(size_t)j + 1]; ++g)
      if (cnt[(size_t)g] > most) most = cnt[(size_t)g], ref = g;
    check("reference group", pl.ref_group[(size_t)j] == ref);
  }
  std::set<int32_t> seen;
  for (size_t a = 0; a < pl.active.size(); ++a) {
    check("queue not empty", pl.q_start[a] < pl.q_start[a + 1]);
    for (int32_t i = pl.q_start[a]; i < pl.q_start[a + 1]; ++i) {
      const pe::BestFitCand e = pl.queue[(size_t)i];
      check("queue entry", pj[(size_t)e.pair] == e.job && pd[(size_t)e.pair] == pl.active[a] && !pl.repeat[(size_t)e.pair] &&
                               seen.insert(e.pair).second);
      check("queue order", i == pl.q_start[a] || pl.rank[(size_t)pl.queue[(size_t)i - 1].job] < pl.rank[(size_t)e.job]);
    }
  }
  check("every kept pair queued", seen.size() == kept);
}

int main() {
  for (unsigned s = 0; s < 60; ++s) verify(s, 1 + (int32_t)(s % 7), 1 + (int32_t)(s % 5), (int32_t)(s * 3 % 41));
  // ---- refusals; the plan stays as it was
  const int32_t off[3] = {0, 1, 3}, pri[2] = {0, 1}, cnt[3] = {2, 1, 3}, sizes[2] = {4, 2}, parent[4] = {0, 0, 1, 1};
  const int32_t pj[4] = {1, 0, 1, 1}, pd[4] = {1, 1, 1, 0};
  BestFitPlan p;
  check("a plan to keep", pe::best_fit_plan_build(p, 2, off, pri, cnt, 4, pj, pd, 1, 2, sizes, parent) == pe::FIT_OK &&
                              p.repeat == std::vector<uint8_t>({0, 0, 1, 0}) && p.kept == Vec({1, 0, 3}) &&
                              p.ref_group == Vec({0, 2}) && p.rank == Vec({1, 0}) && p.active == Vec({0, 1}) &&
                              p.q_start == Vec({0, 1, 3}) && p.queue[0].pair == 3 && p.queue[1].pair == 0 && p.queue[2].pair == 1);
  const BestFitPlan before = p;
  auto refused = [&](const char* name, int64_t n_pairs, const int32_t* j, const int32_t* d, int32_t level, int32_t n_levels,
                     const int32_t* par, pe::FitPlanError want, int64_t want_index) {
    int64_t bad = 99;
    const pe::FitPlanError e = pe::best_fit_plan_build(p, 2, off, pri, cnt, n_pairs, j, d, level, n_levels, sizes, par, nullptr, &bad);
    check(name, e == want && bad == want_index && p.repeat == before.repeat && p.kept == before.kept &&
                    p.kept_start == before.kept_start && p.q_start == before.q_start && p.ref_group == before.ref_group &&
                    p.rank == before.rank && p.queue.size() == before.queue.size() && p.leaf_dom == before.leaf_dom &&
                    p.pod_off == before.pod_off);
    ++refusals;
  };
  const int32_t j_out[4] = {1, 2, 0, 0}, d_out[4] = {1, 0, 2, 0};
  refused("the hierarchy first", 4, j_out, d_out, 5, 2, nullptr, pe::FIT_BAD_TREE, -1);
  refused("level", 4, pj, pd, 2, 2, parent, pe::FIT_BAD_LEVEL, -1);
  refused("pairs NULL", 4, nullptr, pd, 1, 2, parent, pe::FIT_NO_PAIRS, -1);
  refused("pair_job outside", 4, j_out, pd, 1, 2, parent, pe::FIT_BAD_JOB, 1);
  refused("pair_domain outside", 4, pj, d_out, 1, 2, parent, pe::FIT_BAD_DOMAIN, 2);
  printf("%ld plans, %ld refusals, %d failures\n", plans, refusals, failed);
  return failed ? 1 : 0;
}
