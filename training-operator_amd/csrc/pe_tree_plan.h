// The roll-up plan of pe_gang_capacity_tree: a caller's parent map over a hierarchy of topology levels
// (node -> rack -> block -> zone ...) validated and turned into what tree_rollup_kernel (pe_tree.hip)
// reads.  Plain C++, no HIP: the engine builds it on the host once per call, and tests/cpp/test_tree_plan.cc
// builds it under the sanitizers.
//
// Level 0 is the leaf level; level l has size[l] domains, whose table columns are off[l] .. off[l] + size[l]
// - 1 (off[0] = 0, T = the sum of the sizes).  parent[off[l] + k] is the level-(l + 1) domain that holds
// domain k of level l, or -1: the domain counts at its own level and nowhere above.  The top level has no
// entries in the map.
//
// Per upper level l >= 1 the plan holds a CSR over the level's domains: the children of parent p are
//   child[child_at[l] + start[start_at[l] + p]] .. child[child_at[l] + start[start_at[l] + p + 1] - 1],
// level-(l - 1) ids in ASCENDING order, and width[l], the lanes that fold one parent: the smallest power of
// two that covers the level's largest fan-in, 64 at most (wider lists are strided over).  `words` is both
// arrays back to back, the form that crosses to the device in one copy.
#ifndef PE_TREE_PLAN_H_
#define PE_TREE_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace pe {

constexpr int TREE_MAX_LEVELS = 4;           // PE_MAX_LEVELS
constexpr int TREE_MAX_LEVEL_SIZE = 65536;   // PE_MAX_DOMAINS

enum TreePlanError {
  TREE_OK = 0,
  TREE_BAD_LEVELS = 1,   // n_levels outside [1, TREE_MAX_LEVELS]
  TREE_NO_SIZES = 2,     // level_size NULL
  TREE_BAD_SIZE = 3,     // a level size outside [1, TREE_MAX_LEVEL_SIZE]; index = the level
  TREE_NO_PARENT = 4,    // parent NULL with n_levels > 1
  TREE_BAD_PARENT = 5    // a parent outside [-1, size of the level above); index = its place in the map
};

struct TreePlan {
  int32_t n_levels = 0;
  int32_t size[TREE_MAX_LEVELS] = {0, 0, 0, 0};
  int32_t off[TREE_MAX_LEVELS + 1] = {0, 0, 0, 0, 0};   // off[n_levels] = T
  int32_t width[TREE_MAX_LEVELS] = {0, 0, 0, 0};        // levels 1 ..: lanes per parent (1 .. 64)
  int32_t fan_in[TREE_MAX_LEVELS] = {0, 0, 0, 0};       // levels 1 ..: the largest child count
  int32_t start_at[TREE_MAX_LEVELS] = {0, 0, 0, 0};     // levels 1 ..: where the level's start[size + 1] begins in words
  int32_t child_at[TREE_MAX_LEVELS] = {0, 0, 0, 0};     // levels 1 ..: where its child list begins in words
  std::vector<int32_t> words;                           // per upper level: start[size[l] + 1], then the children

  int64_t columns() const { return off[n_levels]; }
  int64_t upper_columns() const { return off[n_levels] - size[0]; }
};

// Lanes per parent for a level whose largest fan-in is f.
inline int32_t tree_width(int32_t f) {
  int32_t w = 1;
  while (w < f && w < 64) w <<= 1;
  return w;
}

// Builds the plan.  On any error `plan` is left exactly as it was and *bad_index (if given) receives the
// first offending index, -1 where the error has none.
inline TreePlanError tree_plan_build(TreePlan& plan, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                     int64_t* bad_index = nullptr) {
  auto fail = [&](TreePlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  if (n_levels < 1 || n_levels > TREE_MAX_LEVELS) return fail(TREE_BAD_LEVELS, -1);
  if (!level_size) return fail(TREE_NO_SIZES, -1);
  for (int l = 0; l < n_levels; ++l)
    if (level_size[l] < 1 || level_size[l] > TREE_MAX_LEVEL_SIZE) return fail(TREE_BAD_SIZE, l);
  if (n_levels > 1 && !parent) return fail(TREE_NO_PARENT, -1);
  TreePlan p;
  p.n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    p.size[l] = level_size[l];
    p.off[l + 1] = p.off[l] + level_size[l];
  }
  for (int l = 0; l + 1 < n_levels; ++l)
    for (int32_t k = 0; k < p.size[l]; ++k) {
      const int32_t v = parent[p.off[l] + k];
      if (v < -1 || v >= p.size[l + 1]) return fail(TREE_BAD_PARENT, (int64_t)p.off[l] + k);
    }
  size_t total = 0;
  for (int l = 1; l < n_levels; ++l) total += (size_t)p.size[l] + 1 + (size_t)p.size[l - 1];
  p.words.assign(total, 0);
  int32_t at = 0;
  for (int l = 1; l < n_levels; ++l) {
    const int32_t* par = parent + p.off[l - 1];
    const int32_t nc = p.size[l - 1], np = p.size[l];
    p.start_at[l] = at;
    p.child_at[l] = at + np + 1;
    int32_t* start = p.words.data() + p.start_at[l];
    int32_t* child = p.words.data() + p.child_at[l];
    // counting sort by parent: ascending child ids within a parent
    for (int32_t c = 0; c < nc; ++c)
      if (par[c] >= 0) ++start[par[c] + 1];
    int32_t f = 0;
    for (int32_t q = 0; q < np; ++q) {
      if (start[q + 1] > f) f = start[q + 1];
      start[q + 1] += start[q];
    }
    std::vector<int32_t> fill(start, start + np);
    for (int32_t c = 0; c < nc; ++c)
      if (par[c] >= 0) child[fill[(size_t)par[c]]++] = c;
    p.fan_in[l] = f;
    p.width[l] = tree_width(f);
    at += np + 1 + nc;   // the child list keeps nc places: those past start[np] are unused
  }
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return TREE_OK;
}

}  // namespace pe

#endif  // PE_TREE_PLAN_H_
