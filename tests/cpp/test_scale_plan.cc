// The plan of pe_scale_up_domains (training-operator_amd/csrc/pe_scale_plan.h): everything but the units against
// fit_plan_build on the same pairs, the per-pair maxima in plan order, the units by weight against the properties
// that determine the greedy cut (found by a scan per domain), the weight bound of every unit, and every refusal with
// its index, each leaving the plan as it was.  Built and run by tests/test_scale_plan_cpu.py with g++ and the address
// and undefined-behaviour sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "pe_scale_plan.h"

using pe::FitPlan;
using pe::ScalePlan;

static int failed = 0;
static long plans = 0, units_checked = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_units(const std::vector<pe::FitUnit>& a, const std::vector<pe::FitUnit>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].act != b[i].act || a[i].p0 != b[i].p0 || a[i].p1 != b[i].p1) return false;
  return true;
}

static bool same_plan(const ScalePlan& a, const ScalePlan& b) {
  return a.kmax == b.kmax && a.fit.level == b.fit.level && a.fit.n_leaf == b.fit.n_leaf && a.fit.n_dom == b.fit.n_dom &&
         a.fit.leaf_dom == b.fit.leaf_dom && a.fit.act_of == b.fit.act_of && a.fit.active == b.fit.active &&
         a.fit.pair_start == b.fit.pair_start && a.fit.pairs == b.fit.pairs && a.fit.unit_start == b.fit.unit_start &&
         same_units(a.fit.units, b.fit.units);
}

// One call's arguments.  Nodes [0, n_total); node n is a removed slot iff removed.count(n).
struct Call {
  int64_t n_jobs = 4, n_total = 100;
  std::vector<int64_t> tmpl = {8, 8, 8, 8, 4, 4, 4, 4};
  int32_t n_templates = 2;
  std::vector<int32_t> slots = {90, 3, 50, 91};
  int32_t n_new = 4;
  std::vector<int32_t> job = {0, 1, 2, 3, 0}, domain = {0, 1, 1, 2, 1}, tmpl_of = {0, 1, 0, 1, 1}, kmax = {0, 4, 2, 1, 3};
  bool with_max = true;
  std::vector<int32_t> sizes = {4, 2, 1}, parent = {0, 0, 1, -1, 0, 0};
  int32_t level = 0;
  std::set<int32_t> removed = {3, 50, 90, 91, 92};
};

static pe::ScalePlanError build(ScalePlan& plan, const Call& c, int64_t* bad, pe::FitPlanError* fe = nullptr,
                                pe::TreePlanError* te = nullptr, bool null_tmpl = false, bool null_slots = false,
                                bool null_pair_tmpl = false) {
  return pe::scale_plan_build(
      plan, c.n_jobs, c.n_total, c.n_templates, null_tmpl ? nullptr : c.tmpl.data(), c.n_new,
      null_slots ? nullptr : c.slots.data(), (int64_t)c.job.size(), c.job.data(), c.domain.data(),
      null_pair_tmpl ? nullptr : c.tmpl_of.data(), c.with_max ? c.kmax.data() : nullptr, c.level, (int32_t)c.sizes.size(),
      c.sizes.data(), c.parent.empty() ? nullptr : c.parent.data(), [&](int32_t n) { return c.removed.count(n) != 0; }, fe,
      te, bad);
}

// A plan that was built against what the fit plan and a scan per domain say.
static void verify(const char* name, const Call& c) {
  ScalePlan p;
  int64_t bad = 7;
  pe::FitPlanError fe = pe::FIT_BAD_JOB;
  pe::TreePlanError te = pe::TREE_BAD_LEVELS;
  const pe::ScalePlanError e = build(p, c, &bad, &fe, &te);
  check(name, e == pe::SCALE_OK && fe == pe::FIT_OK && te == pe::TREE_OK && bad == -1);
  if (e != pe::SCALE_OK) return;
  ++plans;
  FitPlan f;
  const int64_t P = (int64_t)c.job.size();
  check(name, pe::fit_plan_build(f, c.n_jobs, P, c.job.data(), c.domain.data(), c.level, (int32_t)c.sizes.size(),
                                 c.sizes.data(), c.parent.empty() ? nullptr : c.parent.data()) == pe::FIT_OK);
  check(name, p.fit.level == f.level && p.fit.n_leaf == f.n_leaf && p.fit.n_dom == f.n_dom && p.fit.leaf_dom == f.leaf_dom &&
                  p.fit.act_of == f.act_of && p.fit.active == f.active && p.fit.pair_start == f.pair_start &&
                  p.fit.pairs == f.pairs);
  check(name, (int64_t)p.kmax.size() == P);
  for (int64_t i = 0; i < P && i < (int64_t)p.kmax.size(); ++i)
    check(name, p.kmax[(size_t)i] == (c.with_max ? c.kmax[(size_t)p.fit.pairs[(size_t)i]] : c.n_new));
  // the units: per domain they cover its range in order without gaps; a unit of several pairs weighs at most
  // SCALE_UNIT_WEIGHT; no unit weighs more than 65; and a unit could not have taken the next one's first pair
  const size_t A = p.fit.active.size();
  check(name, p.fit.unit_start.size() == A + 1 && p.fit.unit_start[0] == 0 &&
                  p.fit.unit_start[A] == (int32_t)p.fit.units.size());
  auto weight = [&](int32_t p0, int32_t p1) {
    int64_t w = 0;
    for (int32_t i = p0; i < p1; ++i) w += p.kmax[(size_t)i] + 1;
    return w;
  };
  bool all_zero = true;
  for (int32_t k : p.kmax) all_zero &= k == 0;
  for (size_t a = 0; a < A; ++a) {
    int32_t at = p.fit.pair_start[a];
    for (int32_t u = p.fit.unit_start[a]; u < p.fit.unit_start[a + 1]; ++u) {
      const pe::FitUnit& un = p.fit.units[(size_t)u];
      ++units_checked;
      check(name, un.act == (int32_t)a && un.p0 == at && un.p1 > un.p0 && un.p1 <= p.fit.pair_start[a + 1]);
      const int64_t w = weight(un.p0, un.p1);
      check(name, w <= pe::SCALE_MAX_NEW + 1 || un.p1 - un.p0 > 1);
      check(name, un.p1 - un.p0 == 1 || w <= pe::SCALE_UNIT_WEIGHT);
      check(name, w <= std::max(pe::SCALE_UNIT_WEIGHT, pe::SCALE_MAX_NEW + 1));
      if (u + 1 < p.fit.unit_start[a + 1]) check(name, w + p.kmax[(size_t)un.p1] + 1 > pe::SCALE_UNIT_WEIGHT);
      at = un.p1;
    }
    check(name, at == p.fit.pair_start[a + 1]);
  }
  if (all_zero) check(name, same_units(p.fit.units, f.units) && p.fit.unit_start == f.unit_start);
}

// A refusal: the error, its index, and the plan as it was.
static void refuse(const char* name, const Call& c, pe::ScalePlanError want, int64_t want_bad, bool null_tmpl = false,
                   bool null_slots = false, bool null_pair_tmpl = false) {
  ScalePlan p, before;
  int64_t bad = 7;
  check(name, build(p, Call(), &bad) == pe::SCALE_OK);
  before = p;
  bad = 7;
  const pe::ScalePlanError e = build(p, c, &bad, nullptr, nullptr, null_tmpl, null_slots, null_pair_tmpl);
  check(name, e == want);
  check(name, bad == want_bad);
  check(name, same_plan(p, before));
  ++refusals;
}

int main() {
  std::mt19937 rng(20261021);
  verify("default", Call());
  for (int it = 0; it < 400; ++it) {
    Call c;
    c.n_new = (int32_t)(rng() % 65);
    if (it % 7 == 0) c.n_new = 64;
    if (it % 11 == 0) c.n_new = 0;
    c.n_total = 300;
    c.removed.clear();
    c.slots.clear();
    while ((int32_t)c.slots.size() < c.n_new) {
      const int32_t s = (int32_t)(rng() % 300);
      if (c.removed.insert(s).second) c.slots.push_back(s);
    }
    c.sizes = {40, 8, 1};
    c.parent.clear();
    for (int k = 0; k < 40; ++k) c.parent.push_back(k % 9 == 8 ? -1 : k / 5);
    for (int k = 0; k < 8; ++k) c.parent.push_back(0);
    c.level = (int32_t)(rng() % 3);
    const int32_t n_dom = c.sizes[(size_t)c.level];
    const int P = it % 5 == 0 ? (int)(rng() % 4) : (int)(rng() % 400);
    c.n_jobs = 1 + (int64_t)(rng() % 20);
    c.job.clear(), c.domain.clear(), c.tmpl_of.clear(), c.kmax.clear();
    const int mode = it % 4;   // 0: any maximum, 1: all 0, 2: small ones, 3: NULL
    for (int i = 0; i < P; ++i) {
      c.job.push_back((int32_t)(rng() % (uint32_t)c.n_jobs));
      c.domain.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
      c.tmpl_of.push_back((int32_t)(rng() % 2));
      c.kmax.push_back(mode == 1 ? 0 : (int32_t)(rng() % (uint32_t)((mode == 2 ? std::min(c.n_new, 3) : c.n_new) + 1)));
    }
    c.with_max = mode != 3;
    verify("random", c);
  }
  {   // the cut at the boundary weights: 32 pairs of weight 1; 33; weights that add up to 32 exactly and to 33
    Call c;
    c.sizes = {1};
    c.parent.clear();
    c.n_jobs = 1;
    for (int P : {32, 33, 64, 65}) {
      c.job.assign((size_t)P, 0), c.domain.assign((size_t)P, 0), c.tmpl_of.assign((size_t)P, 0), c.kmax.assign((size_t)P, 0);
      verify("flat", c);
      ScalePlan p;
      int64_t bad;
      check("flat units", build(p, c, &bad) == pe::SCALE_OK && (int)p.fit.units.size() == (P + 31) / 32);
    }
    c.job.assign(3, 0), c.domain.assign(3, 0), c.tmpl_of.assign(3, 0);
    c.n_new = 64;
    c.slots.clear(), c.removed.clear();
    for (int32_t s = 0; s < 64; ++s) c.slots.push_back(s + 10), c.removed.insert(s + 10);
    ScalePlan p;
    int64_t bad;
    c.kmax = {15, 15, 0};   // 16 + 16 = 32: one unit, then the third pair
    check("exact", build(p, c, &bad) == pe::SCALE_OK && p.fit.units.size() == 2 && p.fit.units[0].p1 == 2);
    c.kmax = {15, 16, 0};   // 16 + 17 = 33: cut after the first
    check("over", build(p, c, &bad) == pe::SCALE_OK && p.fit.units.size() == 2 && p.fit.units[0].p1 == 1);
    c.kmax = {64, 64, 0};   // heavy pairs alone
    check("heavy", build(p, c, &bad) == pe::SCALE_OK && p.fit.units.size() == 3);
    verify("heavy", c);
  }
  {   // empty calls
    Call c;
    c.job.clear(), c.domain.clear(), c.tmpl_of.clear(), c.kmax.clear();
    verify("no pairs", c);
    c.n_templates = 0;
    c.n_new = 0;
    c.n_jobs = 0;
    verify("nothing", c);
  }
  // ---- every refusal, in the order of the checks, with its index
  {
    Call c;
    c.level = 3;
    refuse("level", c, pe::SCALE_BAD_FIT, -1);
    c = Call();
    c.sizes[1] = 0;
    refuse("tree", c, pe::SCALE_BAD_FIT, 1);
    c = Call();
    c.job[2] = 4;
    refuse("pair_job", c, pe::SCALE_BAD_FIT, 2);
    c = Call();
    c.domain[3] = 4;
    c.n_templates = -1;   // the earlier check wins
    refuse("pair_domain", c, pe::SCALE_BAD_FIT, 3);
    c = Call();
    c.n_templates = -1;
    refuse("n_templates < 0", c, pe::SCALE_BAD_TEMPLATES, -1);
    c.n_templates = 0;
    refuse("no template with pairs", c, pe::SCALE_BAD_TEMPLATES, -1);
    c = Call();
    refuse("tmpl_res NULL", c, pe::SCALE_NO_TEMPLATES, -1, true);
    c.tmpl[6] = -1;
    c.n_new = 65;
    refuse("tmpl_res negative", c, pe::SCALE_BAD_TMPL_RES, 1);
    c.tmpl[3] = INT64_MIN;
    refuse("tmpl_res negative, first", c, pe::SCALE_BAD_TMPL_RES, 0);
    c = Call();
    c.n_new = -1;
    refuse("n_new < 0", c, pe::SCALE_BAD_NEW, -1);
    c.n_new = 65;
    refuse("n_new > 64", c, pe::SCALE_BAD_NEW, -1);
    c = Call();
    refuse("new_slot NULL", c, pe::SCALE_NO_NEW, -1, false, true);
    c.slots[1] = -1;
    refuse("new_slot < 0", c, pe::SCALE_BAD_SLOT, 1);
    c.slots[1] = 100;
    refuse("new_slot >= n_total", c, pe::SCALE_BAD_SLOT, 1);
    c.slots[1] = 4;
    c.slots[3] = 90;   // the live slot comes first
    refuse("new_slot live", c, pe::SCALE_LIVE_SLOT, 1);
    c = Call();
    c.slots[3] = 90;
    refuse("new_slot repeated", c, pe::SCALE_DUP_SLOT, 3);
    c.slots[2] = 3;    // the earlier repetition wins
    refuse("new_slot repeated, first", c, pe::SCALE_DUP_SLOT, 2);
    c = Call();
    refuse("pair_template NULL", c, pe::SCALE_NO_PAIR_TMPL, -1, false, false, true);
    c.tmpl_of[4] = 2;
    c.kmax[0] = 9;
    refuse("pair_template high", c, pe::SCALE_BAD_PAIR_TMPL, 4);
    c.tmpl_of[1] = -1;
    refuse("pair_template low", c, pe::SCALE_BAD_PAIR_TMPL, 1);
    c = Call();
    c.kmax[2] = 5;
    refuse("pair_max > n_new", c, pe::SCALE_BAD_PAIR_MAX, 2);
    c.kmax[0] = -1;
    refuse("pair_max < 0", c, pe::SCALE_BAD_PAIR_MAX, 0);
    c = Call();
    c.n_new = 0;
    refuse("pair_max with no new slot", c, pe::SCALE_BAD_PAIR_MAX, 1);
  }
  printf("%ld plans, %ld units checked, %ld refusals, %d failures\n", plans, units_checked, refusals, failed);
  return failed != 0;
}
