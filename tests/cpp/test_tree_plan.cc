// The roll-up plan of pe_gang_capacity_tree (training-operator_amd/csrc/pe_tree_plan.h): the CSR it makes
// of a parent map against a brute-force grouping, the lanes per parent, and every refusal.  Built and run
// by tests/test_tree_plan_cpu.py with g++ and the address and undefined-behaviour sanitizers: the header
// needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_tree_plan.h"

using pe::TreePlan;

static int failed = 0;
static long plans = 0, parents_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_plan(const TreePlan& a, const TreePlan& b) {
  if (a.n_levels != b.n_levels || a.words != b.words) return false;
  for (int l = 0; l < pe::TREE_MAX_LEVELS; ++l)
    if (a.size[l] != b.size[l] || a.off[l] != b.off[l] || a.width[l] != b.width[l] || a.fan_in[l] != b.fan_in[l] ||
        a.start_at[l] != b.start_at[l] || a.child_at[l] != b.child_at[l])
      return false;
  return a.off[pe::TREE_MAX_LEVELS] == b.off[pe::TREE_MAX_LEVELS];
}

// The plan of (sizes, parent) against the grouping found by scanning the map once per parent.
static void verify(const char* name, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent) {
  TreePlan p;
  int64_t bad = 7;
  const int L = (int)sizes.size();
  const pe::TreePlanError e = pe::tree_plan_build(p, L, sizes.data(), parent.empty() ? nullptr : parent.data(), &bad);
  check(name, e == pe::TREE_OK && bad == -1 && p.n_levels == L);
  if (e != pe::TREE_OK) return;
  ++plans;
  int64_t off = 0, words = 0;
  for (int l = 0; l < L; ++l) {
    check(name, p.size[l] == sizes[l] && p.off[l] == off);
    off += sizes[l];
    if (l > 0) words += (int64_t)sizes[l] + 1 + sizes[l - 1];
  }
  check(name, p.off[L] == off && p.columns() == off && p.upper_columns() == off - sizes[0]);
  check(name, (int64_t)p.words.size() == words);
  for (int l = 1; l < L; ++l) {
    const int32_t* par = parent.data() + p.off[l - 1];
    check(name, p.start_at[l] >= 0 && p.child_at[l] == p.start_at[l] + sizes[l] + 1 &&
                    (size_t)p.child_at[l] + (size_t)sizes[l - 1] <= p.words.size());
    const int32_t* start = p.words.data() + p.start_at[l];
    const int32_t* child = p.words.data() + p.child_at[l];
    check(name, start[0] == 0);
    int32_t fan = 0;
    for (int32_t q = 0; q < sizes[l]; ++q) {
      std::vector<int32_t> want;   // brute force: ascending by construction
      for (int32_t c = 0; c < sizes[l - 1]; ++c)
        if (par[c] == q) want.push_back(c);
      const int32_t b = start[q], e2 = start[q + 1];
      const bool ok = b >= 0 && e2 >= b && e2 <= sizes[l - 1] && (size_t)(e2 - b) == want.size() &&
                      std::equal(want.begin(), want.end(), child + b);
      check(name, ok);
      fan = std::max<int32_t>(fan, (int32_t)want.size());
      ++parents_checked;
    }
    check(name, p.fan_in[l] == fan);
    const int32_t w = p.width[l];
    check(name, w >= 1 && w <= 64 && (w & (w - 1)) == 0 && (w >= fan || w == 64) && (w == 1 || w / 2 < fan));
  }
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

static void refused(const char* name, int32_t n_levels, const int32_t* sizes, const int32_t* parent,
                    pe::TreePlanError want, int64_t want_index) {
  // a plan that holds something: the refusal must leave all of it
  TreePlan p;
  const int32_t s0[3] = {5, 2, 1};
  const int32_t p0[7] = {1, 0, 1, -1, 0, 0, 0};
  check(name, pe::tree_plan_build(p, 3, s0, p0) == pe::TREE_OK);
  const TreePlan before = p;
  int64_t bad = 99;
  const pe::TreePlanError e = pe::tree_plan_build(p, n_levels, sizes, parent, &bad);
  check(name, e == want && bad == want_index && same_plan(p, before));
  check(name, pe::tree_plan_build(p, n_levels, sizes, parent) == want && same_plan(p, before));   // no index asked for
}

int main() {
  // ---- the shapes the engine's tests use
  {
    std::vector<int32_t> p0, p1(20, 0);
    for (int k = 0; k < 79; ++k) p0.push_back(k / 4);
    verify("racks32", {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1, p2(27, 0);
    for (int k = 0; k < 313; ++k) p0.push_back(k / 4);
    for (int k = 0; k < 79; ++k) p1.push_back(k / 3);
    verify("four levels", {313, 79, 27, 1}, concat({p0, p1, p2}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(k % 3 == 1 ? -1 : k / 4);
    for (int k = 0; k < 20; ++k) p1.push_back(k % 2 == 1 ? -1 : 0);
    verify("orphans", {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(2 * (k / 4));
    for (int k = 0; k < 43; ++k) p1.push_back(k % 4 == 0 ? 0 : 2);
    verify("childless parents", {79, 43, 3}, concat({p0, p1}));
  }
  verify("all childless", {6, 3}, {-1, -1, -1, -1, -1, -1});
  verify("one level", {7}, {});
  verify("one level of one", {1}, {});
  {   // the largest level (the brute force is size x size of the level below: a small one above it)
    std::vector<int32_t> p0;
    for (int k = 0; k < 65536; ++k) p0.push_back(k % 7 == 0 ? -1 : (k * 5) % 3);
    verify("largest level", {65536, 3}, p0);
    TreePlan p;
    const int32_t sizes[2] = {3, 65536};
    const int32_t up[3] = {65535, 0, 65535};
    check("largest upper level", pe::tree_plan_build(p, 2, sizes, up) == pe::TREE_OK && p.fan_in[1] == 2 &&
                                     p.width[1] == 2 && p.words[(size_t)p.start_at[1] + 65536] == 3 &&
                                     p.words[(size_t)p.child_at[1]] == 1 && p.words[(size_t)p.child_at[1] + 1] == 0 &&
                                     p.words[(size_t)p.child_at[1] + 2] == 2);
  }
  std::mt19937 rng(5);
  {   // fan-ins 1, 63, 64, 65, 200 in one level, shuffled
    const int fans[5] = {1, 63, 64, 65, 200};
    std::vector<int32_t> p0;
    for (int q = 0; q < 5; ++q) p0.insert(p0.end(), (size_t)fans[q], q);
    std::shuffle(p0.begin(), p0.end(), rng);
    TreePlan p;
    verify("fan-ins", {393, 5, 1}, concat({p0, std::vector<int32_t>(5, 0)}));
    const int32_t sizes[3] = {393, 5, 1};
    const std::vector<int32_t> par = concat({p0, std::vector<int32_t>(5, 0)});
    check("fan-ins width", pe::tree_plan_build(p, 3, sizes, par.data()) == pe::TREE_OK && p.fan_in[1] == 200 &&
                               p.width[1] == 64 && p.fan_in[2] == 5 && p.width[2] == 8);
  }
  // ---- the width per largest fan-in
  const int wf[][2] = {{0, 1}, {1, 1}, {2, 2}, {3, 4}, {4, 4}, {5, 8}, {31, 32}, {32, 32}, {33, 64}, {63, 64}, {64, 64},
                       {65, 64}, {200, 64}, {65536, 64}};
  for (const auto& x : wf) {
    check("tree_width", pe::tree_width(x[0]) == x[1]);
    if (x[0] >= 1 && x[0] <= 300) {
      std::vector<int32_t> par(1, 1);          // leaf 0 -> parent 1, leaves 1 .. f -> parent 0
      par.insert(par.end(), (size_t)x[0], 0);
      TreePlan p;
      const int32_t sizes[2] = {x[0] + 1, 2};
      check("width of a level", pe::tree_plan_build(p, 2, sizes, par.data()) == pe::TREE_OK && p.fan_in[1] == x[0] &&
                                    p.width[1] == x[1]);
      verify("fan tree", {x[0] + 1, 2}, par);
    }
  }
  // ---- random maps: 1 .. 4 levels, random sizes, a fifth of the entries -1
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 4);
    std::vector<int32_t> sizes, par;
    for (int l = 0; l < L; ++l) sizes.push_back(1 + (int32_t)(rng() % (it % 7 == 0 ? 700 : 40)));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < sizes[l]; ++k) par.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)sizes[l + 1]));
    verify("random", sizes, par);
  }
  // ---- refusals: the plan stays as it was
  {
    const int32_t s3[3] = {4, 2, 1};
    const int32_t ok[6] = {0, 1, -1, 1, 0, 0};
    refused("n_levels 0", 0, s3, ok, pe::TREE_BAD_LEVELS, -1);
    refused("n_levels -1", -1, s3, ok, pe::TREE_BAD_LEVELS, -1);
    const int32_t s5[5] = {4, 2, 1, 1, 1};
    refused("n_levels 5", 5, s5, ok, pe::TREE_BAD_LEVELS, -1);
    refused("no sizes", 3, nullptr, ok, pe::TREE_NO_SIZES, -1);
    const int32_t z0[3] = {0, 2, 1}, z1[3] = {4, 0, 1}, z2[3] = {4, 2, -3}, big[3] = {4, 65537, 1};
    refused("level size 0 at the leaves", 3, z0, ok, pe::TREE_BAD_SIZE, 0);
    refused("level size 0 in the middle", 3, z1, ok, pe::TREE_BAD_SIZE, 1);
    refused("negative level size", 3, z2, ok, pe::TREE_BAD_SIZE, 2);
    refused("level size above the limit", 3, big, ok, pe::TREE_BAD_SIZE, 1);
    refused("no parent map", 3, s3, nullptr, pe::TREE_NO_PARENT, -1);
    const int32_t hi[6] = {0, 1, 2, 1, 0, 0}, lo[6] = {0, 1, -2, 1, 0, 0}, top[6] = {0, 1, -1, 1, 0, 1},
                  two[6] = {0, 1, -1, 7, 0, -9};
    refused("parent = the level's size", 3, s3, hi, pe::TREE_BAD_PARENT, 2);
    refused("parent below -1", 3, s3, lo, pe::TREE_BAD_PARENT, 2);
    refused("parent out of range at the second level", 3, s3, top, pe::TREE_BAD_PARENT, 5);
    refused("the first of two bad parents", 3, s3, two, pe::TREE_BAD_PARENT, 3);
    TreePlan one;   // one level: the parent map is not read
    check("one level, no map", pe::tree_plan_build(one, 1, s3, nullptr) == pe::TREE_OK && one.words.empty() &&
                                   one.columns() == 4 && one.upper_columns() == 0);
  }
  printf("%ld plans, %ld parents checked, %d failures\n", plans, parents_checked, failed);
  return failed ? 1 : 0;
}
