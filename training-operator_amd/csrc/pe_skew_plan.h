// The plan of pe_place_skew_domains: pe_place_spread_domains' plan (pe_spread_plan.h: the base plan and, for spread
// domains above the node, leaf_sd / sd_rank / leaf_sub as they are) with what maxSkew adds.  Plain C++, no HIP: the
// engine builds it on the host once per call, and tests/cpp/test_skew_plan.cc builds it under the sanitizers.
//
//   skew[G]          the groups' maxSkew as the kernel reads it: SKEW_FREE (0) for PE_SKEW_NONE
//   book_off[G + 1]  the groups' ranges in the BOOK of existing pods, as the kernel reads it:
//   book[]           (key, count) entries, per group ascending by key with duplicates added up (a sum stops at
//                    2^31 - 1).  The key of an entry is its spread domain: the global node id, or the
//                    level-`spread_level` domain id s -- kept only where s lies under the job's domain, which for a
//                    domain kind the host can tell: (segment, rank) of s is (act_of[anc(s)], sd_rank[s]).  For the
//                    node kind the nodes' leaves are on the device, and the kernel drops an entry whose node has no
//                    place in the job's segment.
//   n_keys           how many keys there are: N nodes or size[spread_level] domains, the length of the call's
//                    key -> place row (skew_scratch_layout)
// The scratch of the call: one row of `sub` words and one of `cnt` words parallel to the segments' places, and the
// key -> place row.
#ifndef PE_SKEW_PLAN_H_
#define PE_SKEW_PLAN_H_

#include "pe_spread_plan.h"

namespace pe {

constexpr int32_t SKEW_NONE = -1;         // PE_SKEW_NONE
constexpr uint32_t SKEW_DRY_RUN = 1u;     // PE_SKEW_DRY_RUN
constexpr int32_t SKEW_FREE = 0;          // skew[g] of an unconstrained group

enum SkewPlanError {
  SKEW_OK = 0,
  SKEW_BAD_PLACE = 1,   // place_plan_build refused: *place_error (and *tree_error) say how
  SKEW_BAD_LEVEL = 2,   // spread_level below -1 or not below level
  SKEW_BAD_SKEW = 3,    // a group_max_skew of 0 or below -1; index = the group
  SKEW_BAD_OFF = 4,     // group_base_off negative or descending at index; -1: entries without base_dom / base_count
  SKEW_BAD_DOM = 5,     // a base_dom outside its level (outside [0, N) for nodes); index = the entry
  SKEW_BAD_COUNT = 6,   // a negative base_count; index = the entry
  SKEW_BAD_FLAGS = 7    // a flags bit the call does not know
};

struct SkewEntry {
  int32_t key, count;
};

struct SkewPlan {
  SpreadPlan sp;
  bool dry_run = false;
  int64_t n_keys = 0;
  std::vector<int32_t> skew, book_off;
  std::vector<SkewEntry> book;

  bool by_node() const { return sp.by_node(); }
  bool constrained() const { return std::any_of(skew.begin(), skew.end(), [](int32_t s) { return s != SKEW_FREE; }); }
};

// Where the call's three scratch rows begin, in 32-bit words, for segments of `stride` places in all.
struct SkewScratch {
  int64_t sub_at, cnt_at, where_at, words;
};
inline SkewScratch skew_scratch_layout(int64_t stride, int64_t n_keys) {
  const int64_t row = (stride + 3) & ~int64_t(3);   // rows start on 16 B
  return SkewScratch{0, row, 2 * row, 2 * row + n_keys};
}

// Builds the plan.  On any error `plan` is left exactly as it was and *bad_index (if given) receives the first
// offending index (-1 where the error has none).  The checks run in this order: the base plan's, spread_level, the
// skews, the book's offsets, its domains, its counts, the flags.  n_nodes: N, the bound of a node-kind base_dom.
inline SkewPlanError skew_plan_build(SkewPlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                     const int32_t* priority, const int32_t* group_count,
                                     const int32_t* group_max_skew, int32_t spread_level, const int32_t* group_base_off,
                                     const int32_t* base_dom, const int32_t* base_count, uint32_t flags,
                                     const int32_t* job_domain, int32_t level, int32_t n_levels,
                                     const int32_t* level_size, const int32_t* parent, int64_t n_nodes,
                                     PlacePlanError* place_error = nullptr, TreePlanError* tree_error = nullptr,
                                     int64_t* bad_index = nullptr) {
  auto fail = [&](SkewPlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  SkewPlan p;
  int64_t bad = -1;
  switch (spread_plan_build(p.sp, n_jobs, job_group_off, priority, group_count, nullptr, spread_level, 0, job_domain,
                            level, n_levels, level_size, parent, place_error, tree_error, &bad)) {
    case SPREAD_OK: break;
    case SPREAD_BAD_PLACE: return fail(SKEW_BAD_PLACE, bad);
    default: return fail(SKEW_BAD_LEVEL, -1);   // no caps and no flags went in
  }
  const int64_t G = n_jobs > 0 ? job_group_off[n_jobs] : 0;
  p.skew.assign((size_t)G, SKEW_FREE);
  if (group_max_skew)
    for (int64_t g = 0; g < G; ++g) {
      const int32_t s = group_max_skew[g];
      if (s == 0 || s < SKEW_NONE) return fail(SKEW_BAD_SKEW, g);
      if (s != SKEW_NONE) p.skew[(size_t)g] = s;
    }
  p.n_keys = p.by_node() ? n_nodes : level_size[spread_level];
  const int64_t E = group_base_off && G > 0 ? group_base_off[G] : 0;
  if (group_base_off) {
    if (G > 0 && group_base_off[0] < 0) return fail(SKEW_BAD_OFF, 0);
    for (int64_t g = 0; g < G; ++g)
      if (group_base_off[g + 1] < group_base_off[g]) return fail(SKEW_BAD_OFF, g + 1);
    if (E > 0 && (!base_dom || !base_count)) return fail(SKEW_BAD_OFF, -1);
    for (int64_t e = group_base_off[0]; G > 0 && e < E; ++e)
      if (base_dom[e] < 0 || base_dom[e] >= p.n_keys) return fail(SKEW_BAD_DOM, e);
    for (int64_t e = group_base_off[0]; G > 0 && e < E; ++e)
      if (base_count[e] < 0) return fail(SKEW_BAD_COUNT, e);
  }
  if (flags & ~SKEW_DRY_RUN) return fail(SKEW_BAD_FLAGS, -1);
  p.dry_run = (flags & SKEW_DRY_RUN) != 0;
  p.book_off.assign((size_t)G + 1, 0);
  if (group_base_off) {
    std::vector<int32_t> anc;   // a spread domain's domain at `level`, walked up the parent map
    if (!p.by_node()) {
      int32_t off = 0;
      for (int l = 0; l < spread_level; ++l) off += level_size[l];
      anc.resize((size_t)level_size[spread_level]);
      std::iota(anc.begin(), anc.end(), 0);
      for (int l = spread_level; l < level; off += level_size[l++])
        for (int32_t& d : anc)
          if (d >= 0) d = parent[off + d];
    }
    std::vector<SkewEntry> own;
    for (int64_t j = 0; j < n_jobs; ++j)
      for (int32_t g = job_group_off[j]; g < job_group_off[j + 1]; ++g) {
        own.clear();
        for (int32_t e = group_base_off[g]; e < group_base_off[g + 1]; ++e)
          if (p.by_node() || anc[(size_t)base_dom[e]] == job_domain[j]) own.push_back(SkewEntry{base_dom[e], base_count[e]});
        std::sort(own.begin(), own.end(), [](const SkewEntry& a, const SkewEntry& b) { return a.key < b.key; });
        for (const SkewEntry& en : own)
          if (!p.book.empty() && (int64_t)p.book.size() > p.book_off[(size_t)g] && p.book.back().key == en.key)
            p.book.back().count = (int32_t)std::min<int64_t>((int64_t)p.book.back().count + en.count, INT32_MAX);
          else
            p.book.push_back(en);
        p.book_off[(size_t)g + 1] = (int32_t)p.book.size();
      }
  }
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return SKEW_OK;
}

}  // namespace pe

#endif  // PE_SKEW_PLAN_H_
