// The plan of pe_place_first_fit_domains (training-operator_amd/csrc/pe_first_fit_plan.h): the ranks, the jobs'
// candidate lists and the domains' queues against a brute force, equal priorities, jobs in no pair, repeated pairs,
// and every refusal.  Built and run by tests/test_first_fit_plan_cpu.py with g++ and the address and
// undefined-behaviour sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <tuple>
#include <vector>

#include "pe_first_fit_plan.h"

using pe::FirstFitPlan;

static int failed = 0;
static long plans = 0, pairs_checked = 0, queues_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_queue(const std::vector<pe::FirstFitCand>& a, const std::vector<pe::FirstFitCand>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].job != b[i].job || a[i].k != b[i].k || a[i].pair != b[i].pair || a[i].last != b[i].last) return false;
  return true;
}

static bool same_plan(const FirstFitPlan& a, const FirstFitPlan& b) {
  return a.level == b.level && a.n_leaf == b.n_leaf && a.n_dom == b.n_dom && a.leaf_dom == b.leaf_dom &&
         a.act_of == b.act_of && a.active == b.active && a.rank == b.rank && a.cand_start == b.cand_start &&
         a.cand == b.cand && a.q_start == b.q_start && same_queue(a.queue, b.queue) && a.pod_off == b.pod_off;
}

struct Batch {
  std::vector<int32_t> off, pri, count, job, domain;   // J jobs with their groups, P pairs
};

// J jobs of 0 .. 3 groups with priorities from a small set (many ties), P pairs in no order with repeats, most of
// them in a few domains, every fourth job in no pair
static Batch random_batch(std::mt19937& rng, int32_t J, int P, int32_t n_dom, bool one_priority = false) {
  Batch b;
  b.off.push_back(0);
  for (int32_t j = 0; j < J; ++j) {
    const int g = (int)(rng() % 4);
    for (int i = 0; i < g; ++i) b.count.push_back((int32_t)(rng() % 5));
    b.off.push_back((int32_t)b.count.size());
    b.pri.push_back(one_priority ? 7 : (int32_t)(rng() % 4) - 1);
  }
  for (int i = 0; i < P; ++i) {
    int32_t j = (int32_t)(rng() % (uint32_t)J);
    if (j % 4 == 3 && J > 1) j = (j + 1) % J;
    b.job.push_back(j);
    b.domain.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
    if (i > 0 && rng() % 6 == 0) {   // the pair before, once more
      b.job.back() = b.job[(size_t)i - 1];
      b.domain.back() = b.domain[(size_t)i - 1];
    }
  }
  return b;
}

// The plan of (hierarchy, level, batch) against what a scan per job, per pair and per domain finds.
static void verify(const char* name, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent, int32_t level,
                   const Batch& b) {
  FirstFitPlan p;
  int64_t bad = 7;
  pe::TreePlanError te = pe::TREE_BAD_LEVELS;
  const int L = (int)sizes.size();
  const int32_t J = (int32_t)b.pri.size();
  const int64_t P = (int64_t)b.job.size();
  const pe::FitPlanError e =
      pe::first_fit_plan_build(p, J, b.off.data(), b.pri.data(), b.count.data(), P, b.job.data(), b.domain.data(), level, L,
                               sizes.data(), parent.empty() ? nullptr : parent.data(), &te, &bad);
  check(name, e == pe::FIT_OK && te == pe::TREE_OK && bad == -1);
  if (e != pe::FIT_OK) return;
  ++plans;
  // the hierarchy's part is pe_gang_fit_domains' plan
  pe::FitPlan f;
  check(name, pe::fit_plan_build(f, J, P, b.job.data(), b.domain.data(), level, L, sizes.data(),
                                 parent.empty() ? nullptr : parent.data()) == pe::FIT_OK);
  check(name, p.level == level && p.n_leaf == sizes[0] && p.n_dom == sizes[(size_t)level] && p.leaf_dom == f.leaf_dom &&
                  p.act_of == f.act_of && p.active == f.active && p.q_start == f.pair_start);
  // ranks: the number of jobs that come before, by (priority desc, index asc)
  check(name, (int32_t)p.rank.size() == J);
  for (int32_t j = 0; j < J && j < (int32_t)p.rank.size(); ++j) {
    int32_t before = 0;
    for (int32_t i = 0; i < J; ++i) before += b.pri[(size_t)i] > b.pri[(size_t)j] || (b.pri[(size_t)i] == b.pri[(size_t)j] && i < j);
    check(name, p.rank[(size_t)j] == before);
  }
  // the jobs' candidates: their pairs in ascending p
  check(name, (int32_t)p.cand_start.size() == J + 1 && (int64_t)p.cand.size() == P && (int64_t)p.queue.size() == P);
  if ((int32_t)p.cand_start.size() != J + 1 || (int64_t)p.cand.size() != P || (int64_t)p.queue.size() != P) return;
  std::vector<int32_t> k_of((size_t)P, -1), n_cand((size_t)J, 0);
  for (int32_t j = 0; j < J; ++j) {
    std::vector<int32_t> want;
    for (int32_t q = 0; q < (int32_t)P; ++q)
      if (b.job[(size_t)q] == j) {
        k_of[(size_t)q] = (int32_t)want.size();
        want.push_back(q);
      }
    n_cand[(size_t)j] = (int32_t)want.size();
    const int32_t s = p.cand_start[(size_t)j], e2 = p.cand_start[(size_t)j + 1];
    check(name, s >= 0 && e2 >= s && e2 <= (int32_t)P && (size_t)(e2 - s) == want.size() &&
                    std::equal(want.begin(), want.end(), p.cand.begin() + s));
    pairs_checked += (long)want.size();
  }
  check(name, p.cand_start[0] == 0 && p.cand_start.back() == (int32_t)P);
  // the queues: every pair of the domain once, sorted by (rank, k), with its position and the last-candidate mark
  const int32_t n_dom = sizes[(size_t)level];
  std::vector<int> seen((size_t)P, 0);
  for (int32_t d = 0; d < n_dom; ++d) {
    std::vector<std::tuple<int32_t, int32_t, int32_t>> want;   // (rank, k, pair)
    for (int32_t q = 0; q < (int32_t)P; ++q)
      if (b.domain[(size_t)q] == d) want.emplace_back(p.rank[(size_t)b.job[(size_t)q]], k_of[(size_t)q], q);
    const int32_t a = p.act_of[(size_t)d];
    if (want.empty()) {
      check(name, a == -1);
      continue;
    }
    std::sort(want.begin(), want.end());
    check(name, a >= 0 && a < (int32_t)p.active.size());
    if (a < 0 || a >= (int32_t)p.active.size()) return;
    const int32_t s = p.q_start[(size_t)a], e2 = p.q_start[(size_t)a + 1];
    check(name, (size_t)(e2 - s) == want.size());
    for (int32_t i = s; i < e2 && (size_t)(i - s) < want.size(); ++i) {
      const pe::FirstFitCand& c = p.queue[(size_t)i];
      const int32_t q = std::get<2>(want[(size_t)(i - s)]);
      check(name, c.pair == q && c.job == b.job[(size_t)q] && c.k == k_of[(size_t)q] &&
                      c.last == (c.k + 1 == n_cand[(size_t)c.job] ? 1 : 0));
      if (c.pair >= 0 && c.pair < (int32_t)P) ++seen[(size_t)c.pair];
    }
    ++queues_checked;
  }
  check(name, std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }));   // every pair in exactly one queue
  // pod slots
  const int32_t G = b.off.back();
  check(name, (int32_t)p.pod_off.size() == G + 1 && p.pod_off[0] == 0);
  int64_t run = 0;
  for (int32_t g = 0; g < G && g + 1 < (int32_t)p.pod_off.size(); ++g) {
    run += b.count[(size_t)g];
    check(name, p.pod_off[(size_t)g + 1] == run);
  }
  check(name, p.pods() == run && p.n_active() == (int64_t)p.active.size());
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

static void all_levels(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes,
                       const std::vector<int32_t>& parent) {
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level)
    verify(name, sizes, parent, level, random_batch(rng, 25, 200, sizes[(size_t)level]));
}

int main() {
  std::mt19937 rng(23);
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
  // ---- by hand: priorities {0, 5, 5, 0}, job 3 in no pair, the pair (1, 2) twice in a row
  {
    const int32_t off[5] = {0, 1, 1, 3, 4}, pri[4] = {0, 5, 5, 0}, count[4] = {2, 0, 3, 1};
    const int32_t pj[6] = {0, 1, 1, 2, 0, 1}, pd[6] = {2, 2, 2, 0, 0, 0}, sizes[1] = {4};
    FirstFitPlan p;
    check("by hand", pe::first_fit_plan_build(p, 4, off, pri, count, 6, pj, pd, 0, 1, sizes, nullptr) == pe::FIT_OK);
    check("by hand: ranks", p.rank == std::vector<int32_t>({2, 0, 1, 3}));
    check("by hand: candidates", p.cand_start == std::vector<int32_t>({0, 2, 5, 6, 6}) &&
                                     p.cand == std::vector<int32_t>({0, 4, 1, 2, 5, 3}));
    check("by hand: domains", p.active == std::vector<int32_t>({0, 2}) && p.q_start == std::vector<int32_t>({0, 3, 6}));
    // domain 0: job 1's third, job 2's only, job 0's second; domain 2: job 1's first and second, job 0's first
    const std::vector<pe::FirstFitCand> want = {{1, 2, 5, 1}, {2, 0, 3, 1}, {0, 1, 4, 1}, {1, 0, 1, 0}, {1, 1, 2, 0}, {0, 0, 0, 0}};
    check("by hand: queues", same_queue(p.queue, want));
    check("by hand: pods", p.pod_off == std::vector<int64_t>({0, 2, 2, 5, 6}));
    // no pairs: a plan without active domains or queues (the pair arrays are not read)
    check("no pairs", pe::first_fit_plan_build(p, 4, off, pri, count, 0, nullptr, nullptr, 0, 1, sizes, nullptr) == pe::FIT_OK &&
                          p.active.empty() && p.queue.empty() && p.cand.empty() && p.q_start == std::vector<int32_t>({0}) &&
                          p.cand_start == std::vector<int32_t>({0, 0, 0, 0, 0}) && p.rank == std::vector<int32_t>({2, 0, 1, 3}));
    check("no jobs, no pairs", pe::first_fit_plan_build(p, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, sizes,
                                                        nullptr) == pe::FIT_OK &&
                                   p.rank.empty() && p.cand_start == std::vector<int32_t>({0}) && p.pods() == 0);
  }
  // ---- equal priorities: the order is the index order
  for (int it = 0; it < 20; ++it) verify("one priority", {40}, {}, 0, random_batch(rng, 30, 150, 40, true));
  // ---- random maps and lists: 1 .. 4 levels, a fifth of the parents -1, every level
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 4);
    std::vector<int32_t> sizes, par;
    for (int l = 0; l < L; ++l) sizes.push_back(1 + (int32_t)(rng() % (it % 7 == 0 ? 700 : 40)));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < sizes[(size_t)l]; ++k)
        par.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)sizes[(size_t)l + 1]));
    const int32_t level = (int32_t)(rng() % (uint32_t)L);
    const int32_t J = 1 + (int32_t)(rng() % 30);
    verify("random", sizes, par, level, random_batch(rng, J, (int)(rng() % (it % 5 == 0 ? 900 : 120)), sizes[(size_t)level]));
  }
  // ---- refusals: the plan stays as it was
  {
    const int32_t s3[3] = {4, 2, 1};
    const int32_t ok[6] = {0, 1, -1, 1, 0, 0};
    const int32_t off[3] = {0, 1, 2}, pri[2] = {1, 2}, count[2] = {3, 4};
    const int32_t job[3] = {1, 0, 1}, dom[3] = {1, 0, 1};
    FirstFitPlan p;
    check("a plan to keep", pe::first_fit_plan_build(p, 2, off, pri, count, 3, job, dom, 1, 3, s3, ok) == pe::FIT_OK);
    const FirstFitPlan before = p;
    auto refused = [&](const char* name, int64_t n_jobs, int64_t n_pairs, const int32_t* pj, const int32_t* pd, int32_t level,
                       int32_t n_levels, const int32_t* sizes, const int32_t* parent, pe::FitPlanError want,
                       pe::TreePlanError want_tree, int64_t want_index) {
      int64_t bad = 99;
      pe::TreePlanError te = pe::TREE_OK;
      const pe::FitPlanError e =
          pe::first_fit_plan_build(p, n_jobs, off, pri, count, n_pairs, pj, pd, level, n_levels, sizes, parent, &te, &bad);
      check(name, e == want && te == want_tree && bad == want_index && same_plan(p, before));
      check(name, pe::first_fit_plan_build(p, n_jobs, off, pri, count, n_pairs, pj, pd, level, n_levels, sizes, parent) == want &&
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
    refused("bad map and bad level", 2, 3, job, dom, 9, 3, s3, hi, pe::FIT_BAD_TREE, pe::TREE_BAD_PARENT, 2);
  }
  printf("%ld plans, %ld pairs, %ld queues checked, %d failures\n", plans, pairs_checked, queues_checked, failed);
  return failed ? 1 : 0;
}
