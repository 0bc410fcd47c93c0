// The plan of pe_place_spread_domains (training-operator_amd/csrc/pe_spread_plan.h): the leaf table, the spread
// domains' ranks and the per-leaf `sub` against a brute force on hand-made hierarchies, the caps, the scratch layout,
// and every refusal, each leaving the plan as it was.  Stand-alone; tests/test_spread_plan_cpu.py builds and runs it.
#include <stdio.h>

#include "pe_spread_plan.h"

using pe::SpreadPlan;
typedef std::vector<int32_t> Vec;

static int failed = 0;
static long plans = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

// Domain k of level `from`, walked up to level `to` one step at a time.
static int32_t walk(const Vec& sizes, const Vec& parent, int32_t k, int from, int to) {
  int32_t off = 0;
  for (int l = 0; l < from; ++l) off += sizes[(size_t)l];
  for (int l = from; l < to && k >= 0; ++l) {
    k = parent[(size_t)(off + k)];
    off += sizes[(size_t)l];
  }
  return k;
}

// Every (level, spread_level) pair of the hierarchy, one job in domain 0 with two groups, caps {3, none}.
static void verify(const char* name, const Vec& sizes, const Vec& parent) {
  const int32_t off[2] = {0, 2}, pri[1] = {0}, cnt[2] = {4, 1}, dom[1] = {0}, caps[2] = {3, pe::SPREAD_NONE};
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level)
    for (int32_t sl = -1; sl < level; ++sl) {
      SpreadPlan p;
      check(name, pe::spread_plan_build(p, 1, off, pri, cnt, caps, sl, sl & 1, dom, level, (int32_t)sizes.size(), sizes.data(),
                                        parent.data()) == pe::SPREAD_OK);
      ++plans;
      check(name, p.by_node() == (sl < 0) && p.dry_run == ((sl & 1) != 0) && p.cap == Vec({3, pe::SPREAD_UNCAPPED}));
      check(name, (int32_t)p.leaf_sub.size() == (sl < 0 ? 0 : sizes[0]) && p.leaf_sd.size() == p.leaf_sub.size() &&
                      (int32_t)p.sd_rank.size() == (sl < 0 ? 0 : sizes[(size_t)sl]));   // per node: no tables
      for (int32_t k = 0; sl >= 0 && k < (int32_t)p.leaf_sub.size(); ++k) {
        const int32_t s = walk(sizes, parent, k, 0, sl);
        int32_t rank = -1;   // the spread domains below s's domain at `level` with a smaller id
        if (s >= 0 && walk(sizes, parent, s, sl, level) >= 0) {
          rank = 0;
          for (int32_t t = 0; t < s; ++t) rank += walk(sizes, parent, t, sl, level) == walk(sizes, parent, s, sl, level);
        }
        check(name, p.leaf_sd[(size_t)k] == s && p.leaf_sub[(size_t)k] == rank && (s < 0 || p.sd_rank[(size_t)s] == rank));
      }
    }
}

int main() {
  // ---- hand-made hierarchies: regular, with orphans at both levels, interleaved parents, four levels
  verify("regular", {6, 3, 1}, {0, 0, 1, 1, 2, 2, 0, 0, 0});
  verify("orphans", {6, 3, 2}, {0, -1, 1, 1, 2, 0, 1, -1, 1});
  verify("interleaved", {7, 4, 2}, {3, 0, 2, 1, 3, 0, 2, 1, 0, 1, 0});
  verify("four levels", {8, 4, 2, 1}, {0, 1, 2, 3, 3, 2, 1, 0, 1, 0, 1, -1, 0, 0});
  const pe::SpreadScratch sa = pe::spread_scratch_layout(1018, true), sb = pe::spread_scratch_layout(1018, false);
  check("scratch", sa.allow_at == 0 && sa.words == 1020 && sb.allow_at == 0 && sb.sub_at == 1020 && sb.words == 2040);
  // ---- refusals, in the order of the checks; the plan stays as it was
  const int32_t off[3] = {0, 1, 3}, pri[2] = {0, 1}, cnt[3] = {2, 1, 3}, dom[2] = {1, 0}, caps[3] = {1, -1, 2};
  const int32_t sizes[3] = {6, 3, 1}, parent[9] = {0, 0, 1, 1, 2, 2, 0, 0, 0};
  SpreadPlan p;
  check("a plan to keep",
        pe::spread_plan_build(p, 2, off, pri, cnt, caps, 0, 0, dom, 1, 3, sizes, parent) == pe::SPREAD_OK &&
            p.leaf_sub == Vec({0, 1, 0, 1, 0, 1}) && p.cap == Vec({1, pe::SPREAD_UNCAPPED, 2}));
  const SpreadPlan before = p;
  auto refused = [&](const char* name, const int32_t* c, int32_t sl, uint32_t flags, const int32_t* d, int32_t level,
                     int32_t n_levels, const int32_t* par, pe::SpreadPlanError want, int64_t want_index,
                     pe::PlacePlanError want_place = pe::PLACE_OK) {
    int64_t bad = 99;
    pe::PlacePlanError pe_ = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    const pe::SpreadPlanError e = pe::spread_plan_build(p, 2, off, pri, cnt, c, sl, flags, d, level, n_levels, sizes, par, &pe_, &te, &bad);
    check(name, e == want && bad == want_index && pe_ == want_place && p.spread_level == before.spread_level && p.dry_run == before.dry_run && p.cap == before.cap &&
                    p.leaf_sub == before.leaf_sub && p.sd_rank == before.sd_rank && p.base.jobs == before.base.jobs);
    ++refusals;
  };
  const int32_t d_hi[2] = {1, 3}, zero[3] = {1, 0, 2}, low[3] = {-2, 0, 2};
  refused("the hierarchy first", zero, 5, 2, dom, 1, 3, nullptr, pe::SPREAD_BAD_PLACE, -1, pe::PLACE_BAD_TREE);
  refused("level", caps, 0, 0, dom, 3, 3, parent, pe::SPREAD_BAD_PLACE, -1, pe::PLACE_BAD_LEVEL);
  refused("job_domain", zero, 1, 2, d_hi, 1, 3, parent, pe::SPREAD_BAD_PLACE, 1, pe::PLACE_BAD_DOMAIN);
  refused("spread_level -2", zero, -2, 2, dom, 1, 3, parent, pe::SPREAD_BAD_LEVEL, -1);
  refused("spread_level = level", zero, 1, 2, dom, 1, 3, parent, pe::SPREAD_BAD_LEVEL, -1);
  refused("spread_level 0 at level 0", caps, 0, 0, dom, 0, 3, parent, pe::SPREAD_BAD_LEVEL, -1);
  refused("cap 0", zero, 0, 2, dom, 1, 3, parent, pe::SPREAD_BAD_CAP, 1);
  refused("cap -2", low, -1, 2, dom, 1, 3, parent, pe::SPREAD_BAD_CAP, 0);
  refused("flags 2", caps, 0, 2, dom, 1, 3, parent, pe::SPREAD_BAD_FLAGS, -1);
  refused("flags high bit", nullptr, -1, 0x80000001u, dom, 1, 3, parent, pe::SPREAD_BAD_FLAGS, -1);
  check("no caps, no jobs", pe::spread_plan_build(p, 0, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, 2, 3, sizes, parent) ==
                                pe::SPREAD_OK && p.cap.empty() && p.dry_run && p.leaf_sub == Vec({0, 0, 1, 1, 2, 2}));
  printf("%ld plans, %ld refusals, %d failures\n", plans, refusals, failed);
  return failed ? 1 : 0;
}
