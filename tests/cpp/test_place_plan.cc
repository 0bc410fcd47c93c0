// The plan of pe_place_greedy_domains (training-operator_amd/csrc/pe_place_plan.h): the leaf -> level map, the
// active domains and their job lists against a brute force, the job order under equal priorities, and every
// refusal.  Built and run by tests/test_place_plan_cpu.py with g++ and the address and undefined-behaviour
// sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_place_plan.h"

using pe::PlacePlan;

static int failed = 0;
static long plans = 0, jobs_checked = 0, leaves_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_plan(const PlacePlan& a, const PlacePlan& b) {
  return a.level == b.level && a.n_leaf == b.n_leaf && a.n_dom == b.n_dom && a.leaf_dom == b.leaf_dom &&
         a.act_of == b.act_of && a.active == b.active && a.job_start == b.job_start && a.jobs == b.jobs &&
         a.pod_off == b.pod_off;
}

struct Batch {
  std::vector<int32_t> off, priority, count, domain;
};

// J jobs of 0 .. 3 groups, priorities from a small set (many ties), domains in [0, n_dom) -- most of them in a
// few domains, so several jobs share one
static Batch random_batch(std::mt19937& rng, int J, int32_t n_dom) {
  Batch b;
  b.off.push_back(0);
  for (int j = 0; j < J; ++j) {
    const int g = (int)(rng() % 4);
    for (int k = 0; k < g; ++k) b.count.push_back((int32_t)(rng() % 5 == 0 ? 0 : rng() % 9));
    b.off.push_back((int32_t)b.count.size());
    b.priority.push_back((int32_t)(rng() % 4) - 1);
    b.domain.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
  }
  return b;
}

// The plan of (hierarchy, level, batch) against what a scan per leaf, per domain and per job finds.
static void verify(const char* name, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent, int32_t level,
                   const Batch& b) {
  PlacePlan p;
  int64_t bad = 7;
  pe::TreePlanError te = pe::TREE_BAD_LEVELS;
  const int L = (int)sizes.size();
  const int64_t J = (int64_t)b.priority.size();
  const pe::PlacePlanError e =
      pe::place_plan_build(p, J, b.off.data(), b.priority.data(), b.count.data(), b.domain.data(), level, L, sizes.data(),
                           parent.empty() ? nullptr : parent.data(), &te, &bad);
  check(name, e == pe::PLACE_OK && te == pe::TREE_OK && bad == -1);
  if (e != pe::PLACE_OK) return;
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
    ++leaves_checked;
  }
  // active domains: ascending, exactly those some job names
  const int32_t n_dom = sizes[(size_t)level];
  check(name, (int32_t)p.act_of.size() == n_dom && p.job_start.size() == p.active.size() + 1 &&
                  (int64_t)p.jobs.size() == J && p.n_active() == (int64_t)p.active.size());
  int32_t a = 0;
  for (int32_t d = 0; d < n_dom; ++d) {
    const bool named = std::find(b.domain.begin(), b.domain.end(), d) != b.domain.end();
    if (named) {
      check(name, a < (int32_t)p.active.size() && p.active[(size_t)a] == d && p.act_of[(size_t)d] == a);
      // the domain's jobs in (priority desc, index asc) order: selection by brute force
      std::vector<int32_t> want;
      for (int32_t j = 0; j < (int32_t)J; ++j)
        if (b.domain[(size_t)j] == d) want.push_back(j);
      std::stable_sort(want.begin(), want.end(),
                       [&](int32_t x, int32_t y) { return b.priority[(size_t)x] > b.priority[(size_t)y]; });
      const int32_t s = p.job_start[(size_t)a], e2 = p.job_start[(size_t)a + 1];
      check(name, s >= 0 && e2 >= s && e2 <= (int32_t)J && (size_t)(e2 - s) == want.size() &&
                      std::equal(want.begin(), want.end(), p.jobs.begin() + s));
      jobs_checked += (long)want.size();
      ++a;
    } else {
      check(name, p.act_of[(size_t)d] == -1);
    }
  }
  check(name, a == (int32_t)p.active.size() && p.job_start[0] == 0 && p.job_start.back() == (int32_t)J);
  // pod offsets
  check(name, p.pod_off.size() == b.count.size() + 1 && p.pod_off[0] == 0);
  int64_t at = 0;
  for (size_t g = 0; g < b.count.size() && g + 1 < p.pod_off.size(); ++g) {
    at += b.count[g];
    check(name, p.pod_off[g + 1] == at);
  }
  check(name, p.pods() == at);
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

static void all_levels(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes,
                       const std::vector<int32_t>& parent) {
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level)
    verify(name, sizes, parent, level, random_batch(rng, 40, sizes[(size_t)level]));
}

int main() {
  std::mt19937 rng(17);
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
  // ---- job order under equal priorities: index ascending; one domain, then two
  {
    Batch b;
    b.off = {0, 1, 1, 2, 3, 3, 4};
    b.count = {2, 0, 5, 1};
    b.priority = {3, 3, 3, 7, 3, 7};
    b.domain = {1, 1, 1, 1, 1, 1};
    PlacePlan p;
    const int32_t sizes[1] = {4};
    check("ties", pe::place_plan_build(p, 6, b.off.data(), b.priority.data(), b.count.data(), b.domain.data(), 0, 1, sizes,
                                       nullptr) == pe::PLACE_OK &&
                      p.jobs == std::vector<int32_t>({3, 5, 0, 1, 2, 4}) && p.active == std::vector<int32_t>({1}) &&
                      p.job_start == std::vector<int32_t>({0, 6}) && p.act_of == std::vector<int32_t>({-1, 0, -1, -1}) &&
                      p.pod_off == std::vector<int64_t>({0, 2, 2, 7, 8}));
    b.domain = {3, 0, 3, 0, 0, 3};
    check("ties in two domains",
          pe::place_plan_build(p, 6, b.off.data(), b.priority.data(), b.count.data(), b.domain.data(), 0, 1, sizes, nullptr) ==
                  pe::PLACE_OK &&
              p.jobs == std::vector<int32_t>({3, 1, 4, 5, 0, 2}) && p.active == std::vector<int32_t>({0, 3}) &&
              p.job_start == std::vector<int32_t>({0, 3, 6}));
    verify("ties, brute force", {4}, {}, 0, b);
    // no jobs: a plan without active domains (job_domain is not read)
    check("no jobs", pe::place_plan_build(p, 0, nullptr, nullptr, nullptr, nullptr, 0, 1, sizes, nullptr) == pe::PLACE_OK &&
                         p.active.empty() && p.jobs.empty() && p.job_start == std::vector<int32_t>({0}) && p.pods() == 0 &&
                         p.leaf_dom == std::vector<int32_t>({0, 1, 2, 3}));
  }
  // ---- random maps and batches: 1 .. 4 levels, a fifth of the parents -1, every level
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 4);
    std::vector<int32_t> sizes, par;
    for (int l = 0; l < L; ++l) sizes.push_back(1 + (int32_t)(rng() % (it % 7 == 0 ? 700 : 40)));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < sizes[(size_t)l]; ++k)
        par.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)sizes[(size_t)l + 1]));
    const int32_t level = (int32_t)(rng() % (uint32_t)L);
    verify("random", sizes, par, level, random_batch(rng, 1 + (int)(rng() % 60), sizes[(size_t)level]));
  }
  // ---- refusals: the plan stays as it was
  {
    const int32_t s3[3] = {4, 2, 1};
    const int32_t ok[6] = {0, 1, -1, 1, 0, 0};
    Batch b;
    b.off = {0, 1, 2};
    b.count = {1, 2};
    b.priority = {0, 0};
    b.domain = {1, 0};
    PlacePlan p;
    check("a plan to keep", pe::place_plan_build(p, 2, b.off.data(), b.priority.data(), b.count.data(), b.domain.data(), 1, 3,
                                                 s3, ok) == pe::PLACE_OK);
    const PlacePlan before = p;
    auto refused = [&](const char* name, const int32_t* domain, int32_t level, int32_t n_levels, const int32_t* sizes,
                       const int32_t* parent, pe::PlacePlanError want, pe::TreePlanError want_tree, int64_t want_index) {
      int64_t bad = 99;
      pe::TreePlanError te = pe::TREE_OK;
      const pe::PlacePlanError e = pe::place_plan_build(p, 2, b.off.data(), b.priority.data(), b.count.data(), domain, level,
                                                        n_levels, sizes, parent, &te, &bad);
      check(name, e == want && te == want_tree && bad == want_index && same_plan(p, before));
      check(name, pe::place_plan_build(p, 2, b.off.data(), b.priority.data(), b.count.data(), domain, level, n_levels, sizes,
                                       parent) == want &&
                      same_plan(p, before));   // nothing asked for
    };
    const int32_t d_hi[2] = {1, 2}, d_lo[2] = {-1, 0}, d_leaf[2] = {3, 4};
    refused("level -1", b.domain.data(), -1, 3, s3, ok, pe::PLACE_BAD_LEVEL, pe::TREE_OK, -1);
    refused("level = n_levels", b.domain.data(), 3, 3, s3, ok, pe::PLACE_BAD_LEVEL, pe::TREE_OK, -1);
    refused("no job_domain", nullptr, 1, 3, s3, ok, pe::PLACE_NO_DOMAINS, pe::TREE_OK, -1);
    refused("domain = the level's size", d_hi, 1, 3, s3, ok, pe::PLACE_BAD_DOMAIN, pe::TREE_OK, 1);
    refused("negative domain", d_lo, 1, 3, s3, ok, pe::PLACE_BAD_DOMAIN, pe::TREE_OK, 0);
    refused("domain = the leaf level's size", d_leaf, 0, 3, s3, ok, pe::PLACE_BAD_DOMAIN, pe::TREE_OK, 1);
    refused("a leaf id at the top level", d_leaf, 2, 3, s3, ok, pe::PLACE_BAD_DOMAIN, pe::TREE_OK, 0);
    // everything tree_plan_build refuses, with its own error and index
    const int32_t s5[5] = {4, 2, 1, 1, 1}, z1[3] = {4, 0, 1}, big[3] = {4, 65537, 1};
    const int32_t hi[6] = {0, 1, 2, 1, 0, 0}, top[6] = {0, 1, -1, 1, 0, 1};
    refused("n_levels 0", b.domain.data(), 0, 0, s3, ok, pe::PLACE_BAD_TREE, pe::TREE_BAD_LEVELS, -1);
    refused("n_levels 5", b.domain.data(), 0, 5, s5, ok, pe::PLACE_BAD_TREE, pe::TREE_BAD_LEVELS, -1);
    refused("no sizes", b.domain.data(), 0, 3, nullptr, ok, pe::PLACE_BAD_TREE, pe::TREE_NO_SIZES, -1);
    refused("level size 0", b.domain.data(), 0, 3, z1, ok, pe::PLACE_BAD_TREE, pe::TREE_BAD_SIZE, 1);
    refused("level size above the limit", b.domain.data(), 0, 3, big, ok, pe::PLACE_BAD_TREE, pe::TREE_BAD_SIZE, 1);
    refused("no parent map", b.domain.data(), 0, 3, s3, nullptr, pe::PLACE_BAD_TREE, pe::TREE_NO_PARENT, -1);
    refused("parent = the level's size", b.domain.data(), 0, 3, s3, hi, pe::PLACE_BAD_TREE, pe::TREE_BAD_PARENT, 2);
    refused("parent out of range at the second level", b.domain.data(), 0, 3, s3, top, pe::PLACE_BAD_TREE,
            pe::TREE_BAD_PARENT, 5);
    // the hierarchy is judged first: a bad level with a bad map names the map
    refused("bad map and bad level", b.domain.data(), 9, 3, s3, hi, pe::PLACE_BAD_TREE, pe::TREE_BAD_PARENT, 2);
  }
  printf("%ld plans, %ld leaves, %ld jobs checked, %d failures\n", plans, leaves_checked, jobs_checked, failed);
  return failed ? 1 : 0;
}
