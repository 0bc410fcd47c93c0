// The plan of pe_place_spread_domains: pe_place_greedy_domains' plan (pe_place_plan.h) with what the per-domain pod
// caps add.  Plain C++, no HIP: the engine builds it on the host once per call, and tests/cpp/test_spread_plan.cc
// builds it under the sanitizers.
//
// The SPREAD DOMAIN of a node is the node itself (spread_level == SPREAD_NODE) or its level-`spread_level` domain,
// 0 <= spread_level < level.  For the second kind the plan holds, beside the base plan,
//   leaf_sd[size[0]]            the level-`spread_level` domain of leaf domain k, walked up the parent map; -1 = none
//   sd_rank[size[spread_level]] the rank of spread domain s among the spread domains that share its level-`level`
//                               domain, ascending ids; -1 where s has no domain at `level`
//   leaf_sub[size[0]]           sd_rank[leaf_sd[k]], -1 where either is none: what a place of a segment carries as
//                               `sub`.  Two places of one segment have equal sub exactly when they share a spread
//                               domain: a segment is one level-`level` domain and the ranks are unique inside it.
//   cap[G]                      the groups' caps as the kernel reads them: SPREAD_UNCAPPED for "no cap".  A group
//                               places at most count <= 2^31 - 1 pods, so that value never binds.
// The scratch of the call (spread_scratch_layout): one row of `allow` words for the segments that do not fit LDS
// and, for the second kind, one row of `sub` words; both run parallel to the segments' places.
#ifndef PE_SPREAD_PLAN_H_
#define PE_SPREAD_PLAN_H_

#include "pe_place_plan.h"

namespace pe {

constexpr int32_t SPREAD_NONE = -1;              // PE_SPREAD_NONE
constexpr int32_t SPREAD_NODE = -1;              // PE_SPREAD_NODE
constexpr uint32_t SPREAD_DRY_RUN = 1u;          // PE_SPREAD_DRY_RUN
constexpr int32_t SPREAD_UNCAPPED = INT32_MAX;

enum SpreadPlanError {
  SPREAD_OK = 0,
  SPREAD_BAD_PLACE = 1,   // place_plan_build refused: *place_error (and *tree_error) say how
  SPREAD_BAD_LEVEL = 2,   // spread_level below -1 or not below level
  SPREAD_BAD_CAP = 3,     // a group_max_per of 0 or below -1; index = the group
  SPREAD_BAD_FLAGS = 4    // a flags bit the call does not know
};

struct SpreadPlan {
  PlacePlan base;
  int32_t spread_level = SPREAD_NODE;
  bool dry_run = false;
  std::vector<int32_t> cap, leaf_sd, sd_rank, leaf_sub;

  bool by_node() const { return spread_level == SPREAD_NODE; }
};

// Where the call's two scratch rows begin, in 32-bit words, for segments of `stride` places in all.
struct SpreadScratch {
  int64_t allow_at, sub_at, words;
};
inline SpreadScratch spread_scratch_layout(int64_t stride, bool by_node) {
  const int64_t row = (stride + 3) & ~int64_t(3);   // rows start on 16 B
  return SpreadScratch{0, by_node ? 0 : row, by_node ? row : 2 * row};
}

// Builds the plan.  On any error `plan` is left exactly as it was and *bad_index (if given) receives the first
// offending index (-1 where the error has none); for SPREAD_BAD_PLACE *place_error and *tree_error say what the
// base plan refused.  The checks run in this order: the base plan's, spread_level, the caps, the flags.
inline SpreadPlanError spread_plan_build(SpreadPlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                         const int32_t* priority, const int32_t* group_count,
                                         const int32_t* group_max_per, int32_t spread_level, uint32_t flags,
                                         const int32_t* job_domain, int32_t level, int32_t n_levels,
                                         const int32_t* level_size, const int32_t* parent,
                                         PlacePlanError* place_error = nullptr, TreePlanError* tree_error = nullptr,
                                         int64_t* bad_index = nullptr) {
  auto fail = [&](SpreadPlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  SpreadPlan p;
  int64_t bad = -1;
  const PlacePlanError pe = place_plan_build(p.base, n_jobs, job_group_off, priority, group_count, job_domain, level,
                                             n_levels, level_size, parent, tree_error, &bad);
  if (place_error) *place_error = pe;
  if (pe != PLACE_OK) return fail(SPREAD_BAD_PLACE, bad);
  if (spread_level < SPREAD_NODE || spread_level >= level) return fail(SPREAD_BAD_LEVEL, -1);
  const int64_t G = n_jobs > 0 ? job_group_off[n_jobs] : 0;
  p.cap.assign((size_t)G, SPREAD_UNCAPPED);
  if (group_max_per)
    for (int64_t g = 0; g < G; ++g) {
      const int32_t m = group_max_per[g];
      if (m == 0 || m < SPREAD_NONE) return fail(SPREAD_BAD_CAP, g);
      if (m != SPREAD_NONE) p.cap[(size_t)g] = m;
    }
  if (flags & ~SPREAD_DRY_RUN) return fail(SPREAD_BAD_FLAGS, -1);
  p.spread_level = spread_level;
  p.dry_run = (flags & SPREAD_DRY_RUN) != 0;
  if (!p.by_node()) {
    int32_t off[TREE_MAX_LEVELS + 1] = {0};   // the hierarchy is valid: the base plan was built
    for (int l = 0; l < n_levels; ++l) off[l + 1] = off[l] + level_size[l];
    const auto up = [&](std::vector<int32_t>& v, int from, int to) {   // one step up the parent map per level
      for (int l = from; l < to; ++l)
        for (int32_t& d : v)
          if (d >= 0) d = parent[off[l] + d];
    };
    p.leaf_sd.resize((size_t)level_size[0]);
    std::iota(p.leaf_sd.begin(), p.leaf_sd.end(), 0);
    up(p.leaf_sd, 0, spread_level);
    std::vector<int32_t> anc((size_t)level_size[spread_level]);   // a spread domain's domain at `level`
    std::iota(anc.begin(), anc.end(), 0);
    up(anc, spread_level, level);
    std::vector<int32_t> next((size_t)level_size[level], 0);
    p.sd_rank.assign(anc.size(), -1);
    for (size_t s = 0; s < anc.size(); ++s)
      if (anc[s] >= 0) p.sd_rank[s] = next[(size_t)anc[s]]++;
    p.leaf_sub.assign(p.leaf_sd.size(), -1);
    for (size_t k = 0; k < p.leaf_sd.size(); ++k)
      if (p.leaf_sd[k] >= 0) p.leaf_sub[k] = p.sd_rank[(size_t)p.leaf_sd[k]];
  }
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return SPREAD_OK;
}

}  // namespace pe

#endif  // PE_SPREAD_PLAN_H_
