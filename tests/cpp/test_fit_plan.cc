// The plan of pe_gang_fit_domains (training-operator_amd/csrc/pe_fit_plan.h): the leaf -> level map, the active
// domains, the pair lists and the work units against a brute force, the unit cuts at the boundary counts, the
// scratch layout's bound, and every refusal.  Built and run by tests/test_fit_plan_cpu.py with g++ and the address
// and undefined-behaviour sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_fit_plan.h"

using pe::FIT_UNIT_PAIRS;
using pe::FitPlan;

static int failed = 0;
static long plans = 0, pairs_checked = 0, units_checked = 0;

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

static bool same_plan(const FitPlan& a, const FitPlan& b) {
  return a.level == b.level && a.n_leaf == b.n_leaf && a.n_dom == b.n_dom && a.leaf_dom == b.leaf_dom &&
         a.act_of == b.act_of && a.active == b.active && a.pair_start == b.pair_start && a.pairs == b.pairs &&
         a.unit_start == b.unit_start && same_units(a.units, b.units);
}

struct Pairs {
  std::vector<int32_t> job, domain;
};

// P pairs over J jobs, most of them in a few domains (so several units share one), in no order, with repeats
static Pairs random_pairs(std::mt19937& rng, int P, int32_t J, int32_t n_dom) {
  Pairs p;
  for (int i = 0; i < P; ++i) {
    p.job.push_back((int32_t)(rng() % (uint32_t)J));
    p.domain.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
  }
  return p;
}

// The plan of (hierarchy, level, pairs) against what a scan per leaf, per domain and per pair finds.
static void verify(const char* name, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent, int32_t level,
                   int32_t J, const Pairs& pr) {
  FitPlan p;
  int64_t bad = 7;
  pe::TreePlanError te = pe::TREE_BAD_LEVELS;
  const int L = (int)sizes.size();
  const int64_t P = (int64_t)pr.job.size();
  const pe::FitPlanError e = pe::fit_plan_build(p, J, P, pr.job.data(), pr.domain.data(), level, L, sizes.data(),
                                                parent.empty() ? nullptr : parent.data(), &te, &bad);
  check(name, e == pe::FIT_OK && te == pe::TREE_OK && bad == -1);
  if (e != pe::FIT_OK) return;
  ++plans;
  check(name, p.level == level && p.n_leaf == sizes[0] && p.n_dom == sizes[(size_t)level]);
  // leaf -> level, one step at a time
  check(name, (int32_t)p.leaf_dom.size() == sizes[0]);
  for (int32_t k = 0; k < sizes[0] && k < (int32_t)p.leaf_dom.size(); ++k) {
    int32_t d = k, off = 0;
    for (int l = 0; l < level && d >= 0; ++l) {
      d = parent[(size_t)(off + d)];
      off += sizes[(size_t)l];
    }
    check(name, p.leaf_dom[(size_t)k] == d);
  }
  // active domains: ascending, exactly those some pair names; their pairs in ascending p
  const int32_t n_dom = sizes[(size_t)level];
  check(name, (int32_t)p.act_of.size() == n_dom && p.pair_start.size() == p.active.size() + 1 &&
                  p.unit_start.size() == p.active.size() + 1 && (int64_t)p.pairs.size() == P);
  std::vector<int> seen((size_t)P, 0);   // how many units hold pair p
  int32_t a = 0;
  for (int32_t d = 0; d < n_dom; ++d) {
    std::vector<int32_t> want;
    for (int32_t q = 0; q < (int32_t)P; ++q)
      if (pr.domain[(size_t)q] == d) want.push_back(q);
    if (want.empty()) {
      check(name, p.act_of[(size_t)d] == -1);
      continue;
    }
    check(name, a < (int32_t)p.active.size() && p.active[(size_t)a] == d && p.act_of[(size_t)d] == a);
    if (a >= (int32_t)p.active.size()) return;
    const int32_t s = p.pair_start[(size_t)a], e2 = p.pair_start[(size_t)a + 1];
    check(name, s >= 0 && e2 >= s && e2 <= (int32_t)P && (size_t)(e2 - s) == want.size() &&
                    std::equal(want.begin(), want.end(), p.pairs.begin() + s));
    pairs_checked += (long)want.size();
    // the domain's units: consecutive runs of its range, all full but the last, none empty
    const int32_t u0 = p.unit_start[(size_t)a], u1 = p.unit_start[(size_t)a + 1];
    const int32_t n_units = ((int32_t)want.size() + FIT_UNIT_PAIRS - 1) / FIT_UNIT_PAIRS;
    check(name, u0 >= 0 && u1 - u0 == n_units && u1 <= (int32_t)p.units.size());
    int32_t at = s;
    for (int32_t u = u0; u < u1 && u < (int32_t)p.units.size(); ++u) {
      const pe::FitUnit& un = p.units[(size_t)u];
      check(name, un.act == a && un.p0 == at && un.p1 > un.p0 && un.p1 <= e2 && un.p1 - un.p0 <= FIT_UNIT_PAIRS &&
                      (un.p1 - un.p0 == FIT_UNIT_PAIRS || u == u1 - 1));
      for (int32_t i = un.p0; i < un.p1 && i < (int32_t)P; ++i) ++seen[(size_t)p.pairs[(size_t)i]];
      at = un.p1;
      ++units_checked;
    }
    check(name, at == e2);
    ++a;
  }
  check(name, a == (int32_t)p.active.size() && p.pair_start[0] == 0 && p.pair_start.back() == (int32_t)P &&
                  p.unit_start[0] == 0 && p.unit_start.back() == (int32_t)p.units.size() && p.n_units() == (int64_t)p.units.size());
  check(name, std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }));   // every pair in exactly one unit
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

static void all_levels(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes,
                       const std::vector<int32_t>& parent) {
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level)
    verify(name, sizes, parent, level, 25, random_pairs(rng, 200, 25, sizes[(size_t)level]));
}

int main() {
  std::mt19937 rng(19);
  // ---- the hierarchies the engine's tests use (tests/tree_capacity.py at 2500 nodes), every level
  {
    std::vector<int32_t> p0, p1(20, 0);
    for (int k = 0; k < 79; ++k) p0.push_back(k / 4);
    all_levels("racks32", rng, {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1, p2(27, 0);
    for (int k = 0; k < 313; ++k) p0.push_back(k / 4);
    for (int k = 0; k < 79; ++k) p1.push_back(k / 3);
    all_levels("four", rng, {313, 79, 27, 1}, concat({p0, p1, p2}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 314; ++k) p0.push_back((int32_t)(rng() % 32));
    for (int k = 0; k < 32; ++k) p1.push_back((int32_t)(rng() % 2));
    all_levels("permuted", rng, {314, 32, 2}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(k % 3 == 1 ? -1 : k / 4);
    for (int k = 0; k < 20; ++k) p1.push_back(k % 2 == 1 ? -1 : 0);
    all_levels("orphans", rng, {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(2 * (k / 4));
    for (int k = 0; k < 43; ++k) p1.push_back(k % 4 == 0 ? 0 : 2);
    all_levels("childless", rng, {79, 43, 3}, concat({p0, p1}));
  }
  {
    const int fans[5] = {1, 63, 64, 65, 200};
    std::vector<int32_t> p0;
    for (int q = 0; q < 5; ++q) p0.insert(p0.end(), (size_t)fans[q], q);
    std::shuffle(p0.begin(), p0.end(), rng);
    all_levels("fanin", rng, {393, 5, 1}, concat({p0, std::vector<int32_t>(5, 0)}));
  }
  all_levels("flat", rng, {79}, {});
  all_levels("largest level", rng, {65536}, {});
  // ---- the unit cuts: domains with 0, 1, U - 1, U, U + 1 and 3 U + 1 pairs, dealt in a shuffled order
  {
    const int U = FIT_UNIT_PAIRS;
    const int counts[6] = {0, 1, U - 1, U, U + 1, 3 * U + 1};
    Pairs pr;
    for (int d = 0; d < 6; ++d)
      for (int i = 0; i < counts[d]; ++i) {
        pr.domain.push_back(d);
        pr.job.push_back((int32_t)(rng() % 9));
      }
    std::shuffle(pr.domain.begin(), pr.domain.end(), rng);
    verify("unit cuts", {6}, {}, 0, 9, pr);
    FitPlan p;
    const int32_t sizes[1] = {6};
    check("unit cuts: the plan",
          pe::fit_plan_build(p, 9, (int64_t)pr.job.size(), pr.job.data(), pr.domain.data(), 0, 1, sizes, nullptr) == pe::FIT_OK &&
              p.active == std::vector<int32_t>({1, 2, 3, 4, 5}) && p.act_of == std::vector<int32_t>({-1, 0, 1, 2, 3, 4}) &&
              p.unit_start == std::vector<int32_t>({0, 1, 2, 3, 5, 9}) &&
              p.pair_start == std::vector<int32_t>({0, 1, U, 2 * U, 3 * U + 1, 6 * U + 2}));
    if (p.units.size() == 9) {
      check("unit cuts: U + 1", p.units[3].p1 - p.units[3].p0 == U && p.units[4].p1 - p.units[4].p0 == 1);
      check("unit cuts: 3 U + 1", p.units[7].p1 - p.units[7].p0 == U && p.units[8].p1 - p.units[8].p0 == 1);
    }
    // no pairs: a plan without active domains or units (the pair arrays are not read)
    check("no pairs", pe::fit_plan_build(p, 9, 0, nullptr, nullptr, 0, 1, sizes, nullptr) == pe::FIT_OK && p.active.empty() &&
                          p.pairs.empty() && p.units.empty() && p.pair_start == std::vector<int32_t>({0}) &&
                          p.unit_start == std::vector<int32_t>({0}) && p.leaf_dom == std::vector<int32_t>({0, 1, 2, 3, 4, 5}));
    check("no jobs, no pairs", pe::fit_plan_build(p, 0, 0, nullptr, nullptr, 0, 1, sizes, nullptr) == pe::FIT_OK);
  }
  // ---- the scratch layout: every large domain at least one copy, never more copies than units, workgroup s of k
  // strides over the domain's units, the copies disjoint and within (1 + FIT_SCRATCH_MULT) * Ns nodes
  for (int it = 0; it < 200; ++it) {
    const int A = 1 + (int)(rng() % 6);
    Pairs pr;
    for (int d = 0; d < A; ++d) {
      const int n = 1 + (int)(rng() % (it % 3 == 0 ? 2000 : 70));
      pr.domain.insert(pr.domain.end(), (size_t)n, d);
      pr.job.insert(pr.job.end(), (size_t)n, 0);
    }
    FitPlan p;
    const int32_t sizes[1] = {A};
    check("layout: plan", pe::fit_plan_build(p, 1, (int64_t)pr.job.size(), pr.job.data(), pr.domain.data(), 0, 1, sizes,
                                             nullptr) == pe::FIT_OK);
    const int lds = 100;
    std::vector<int32_t> seg_off(1, 0);
    for (int d = 0; d < A; ++d) seg_off.push_back(seg_off.back() + (int32_t)(rng() % 2 ? rng() % 100 : 101 + rng() % 5000));
    const int64_t Ns = seg_off.back() + (int64_t)(rng() % 50);
    std::vector<pe::FitLarge> large;
    const int64_t nodes = pe::fit_scratch_layout(p, seg_off.data(), Ns, lds, large);
    check("layout: bound", nodes >= 0 && nodes <= (1 + pe::FIT_SCRATCH_MULT) * Ns);
    int64_t at = 0;
    size_t w = 0;
    for (int d = 0; d < A; ++d) {
      const int64_t n = seg_off[(size_t)d + 1] - seg_off[(size_t)d];
      if (n <= lds) continue;
      const int32_t u0 = p.unit_start[(size_t)d], u1 = p.unit_start[(size_t)d + 1];
      check("layout: a record", w < large.size());
      if (w >= large.size()) break;
      const int32_t k = large[w].k;
      check("layout: copies", k >= 1 && k <= u1 - u0);
      for (int32_t s = 0; s < k && w < large.size(); ++s, ++w) {
        const pe::FitLarge& r = large[w];
        check("layout: record", r.act == d && r.u0 == u0 && r.u1 == u1 && r.k == k && r.s == s && r.at == at);
        at += 4 * n;
      }
    }
    check("layout: all records", w == large.size() && at == 4 * nodes);
  }
  // ---- random maps and pair lists: 1 .. 4 levels, a fifth of the parents -1, every level
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 4);
    std::vector<int32_t> sizes, par;
    for (int l = 0; l < L; ++l) sizes.push_back(1 + (int32_t)(rng() % (it % 7 == 0 ? 700 : 40)));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < sizes[(size_t)l]; ++k)
        par.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)sizes[(size_t)l + 1]));
    const int32_t level = (int32_t)(rng() % (uint32_t)L);
    const int32_t J = 1 + (int32_t)(rng() % 30);
    verify("random", sizes, par, level, J, random_pairs(rng, (int)(rng() % (it % 5 == 0 ? 900 : 120)), J, sizes[(size_t)level]));
  }
  // ---- refusals: the plan stays as it was
  {
    const int32_t s3[3] = {4, 2, 1};
    const int32_t ok[6] = {0, 1, -1, 1, 0, 0};
    const int32_t job[3] = {1, 0, 1}, dom[3] = {1, 0, 1};
    FitPlan p;
    check("a plan to keep", pe::fit_plan_build(p, 2, 3, job, dom, 1, 3, s3, ok) == pe::FIT_OK);
    const FitPlan before = p;
    auto refused = [&](const char* name, int64_t n_jobs, int64_t n_pairs, const int32_t* pj, const int32_t* pd, int32_t level,
                       int32_t n_levels, const int32_t* sizes, const int32_t* parent, pe::FitPlanError want,
                       pe::TreePlanError want_tree, int64_t want_index) {
      int64_t bad = 99;
      pe::TreePlanError te = pe::TREE_OK;
      const pe::FitPlanError e = pe::fit_plan_build(p, n_jobs, n_pairs, pj, pd, level, n_levels, sizes, parent, &te, &bad);
      check(name, e == want && te == want_tree && bad == want_index && same_plan(p, before));
      check(name, pe::fit_plan_build(p, n_jobs, n_pairs, pj, pd, level, n_levels, sizes, parent) == want &&
                      same_plan(p, before));   // nothing asked for
    };
    const int32_t j_hi[3] = {1, 2, 0}, j_lo[3] = {-1, 0, 0}, d_hi[3] = {1, 0, 2}, d_lo[3] = {1, -1, 9}, d_leaf[3] = {0, 3, 4};
    refused("level -1", 2, 3, job, dom, -1, 3, s3, ok, pe::FIT_BAD_LEVEL, pe::TREE_OK, -1);
    refused("level = n_levels", 2, 3, job, dom, 3, 3, s3, ok, pe::FIT_BAD_LEVEL, pe::TREE_OK, -1);
    refused("n_pairs < 0", 2, -1, job, dom, 1, 3, s3, ok, pe::FIT_BAD_COUNT, pe::TREE_OK, -1);
    refused("n_pairs = 2^31 - 1", 2, 2147483647, job, dom, 1, 3, s3, ok, pe::FIT_BAD_COUNT, pe::TREE_OK, -1);
    refused("n_jobs < 0", -1, 3, job, dom, 1, 3, s3, ok, pe::FIT_BAD_COUNT, pe::TREE_OK, -1);
    refused("no pair_job", 2, 3, nullptr, dom, 1, 3, s3, ok, pe::FIT_NO_PAIRS, pe::TREE_OK, -1);
    refused("no pair_domain", 2, 3, job, nullptr, 1, 3, s3, ok, pe::FIT_NO_PAIRS, pe::TREE_OK, -1);
    refused("job = n_jobs", 2, 3, j_hi, dom, 1, 3, s3, ok, pe::FIT_BAD_JOB, pe::TREE_OK, 1);
    refused("negative job", 2, 3, j_lo, dom, 1, 3, s3, ok, pe::FIT_BAD_JOB, pe::TREE_OK, 0);
    refused("a pair with no jobs", 0, 3, job, dom, 1, 3, s3, ok, pe::FIT_BAD_JOB, pe::TREE_OK, 0);
    refused("domain = the level's size", 2, 3, job, d_hi, 1, 3, s3, ok, pe::FIT_BAD_DOMAIN, pe::TREE_OK, 2);
    refused("negative domain", 2, 3, job, d_lo, 1, 3, s3, ok, pe::FIT_BAD_DOMAIN, pe::TREE_OK, 1);
    refused("domain = the leaf level's size", 2, 3, job, d_leaf, 0, 3, s3, ok, pe::FIT_BAD_DOMAIN, pe::TREE_OK, 2);
    refused("a bad job before a bad domain", 2, 3, j_hi, d_lo, 1, 3, s3, ok, pe::FIT_BAD_JOB, pe::TREE_OK, 1);
    // everything tree_plan_build refuses, with its own error and index
    const int32_t s5[5] = {4, 2, 1, 1, 1}, z1[3] = {4, 0, 1}, big[3] = {4, 65537, 1};
    const int32_t hi[6] = {0, 1, 2, 1, 0, 0}, top[6] = {0, 1, -1, 1, 0, 1};
    refused("n_levels 0", 2, 3, job, dom, 0, 0, s3, ok, pe::FIT_BAD_TREE, pe::TREE_BAD_LEVELS, -1);
    refused("n_levels 5", 2, 3, job, dom, 0, 5, s5, ok, pe::FIT_BAD_TREE, pe::TREE_BAD_LEVELS, -1);
    refused("no sizes", 2, 3, job, dom, 0, 3, nullptr, ok, pe::FIT_BAD_TREE, pe::TREE_NO_SIZES, -1);
    refused("level size 0", 2, 3, job, dom, 0, 3, z1, ok, pe::FIT_BAD_TREE, pe::TREE_BAD_SIZE, 1);
    refused("level size above the limit", 2, 3, job, dom, 0, 3, big, ok, pe::FIT_BAD_TREE, pe::TREE_BAD_SIZE, 1);
    refused("no parent map", 2, 3, job, dom, 0, 3, s3, nullptr, pe::FIT_BAD_TREE, pe::TREE_NO_PARENT, -1);
    refused("parent = the level's size", 2, 3, job, dom, 0, 3, s3, hi, pe::FIT_BAD_TREE, pe::TREE_BAD_PARENT, 2);
    refused("parent out of range at the second level", 2, 3, job, dom, 0, 3, s3, top, pe::FIT_BAD_TREE, pe::TREE_BAD_PARENT, 5);
    // the hierarchy is judged first: a bad level with a bad map names the map
    refused("bad map and bad level", 2, 3, job, dom, 9, 3, s3, hi, pe::FIT_BAD_TREE, pe::TREE_BAD_PARENT, 2);
  }
  printf("%ld plans, %ld pairs, %ld units checked, %d failures\n", plans, pairs_checked, units_checked, failed);
  return failed ? 1 : 0;
}
