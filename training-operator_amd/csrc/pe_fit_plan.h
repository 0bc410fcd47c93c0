// The plan of pe_gang_fit_domains: the caller's hierarchy and (job, domain) pair list validated and turned into
// what the kernels of pe_fit.hip read.  Plain C++, no HIP: the engine builds it on the host once per call, and
// tests/cpp/test_fit_plan.cc builds it under the sanitizers.
//
// The hierarchy is pe_gang_capacity_tree's (pe_tree_plan.h validates it).  For the call's `level` the plan holds
//   leaf_dom, act_of, active[A]   pe_domain_map.h's maps; a domain is active when some pair names it
//   pair_start[A + 1], pairs[P]   CSR from active domain to its pairs, ascending p within a domain
//   unit_start[A + 1], units[U]   the WORK UNITS: domain a's CSR range cut into runs of at most FIT_UNIT_PAIRS
//                        places, units[unit_start[a] .. unit_start[a + 1]) in ascending order of the range
// Every pair is judged alone, so a domain's pairs may be judged by many workgroups at once: a rack that is a
// candidate for thousands of gangs is thousands / FIT_UNIT_PAIRS units, not one long chain.
// The batch arrays (offsets monotonic, counts >= 0) are the engine's to check before the plan is built.
#ifndef PE_FIT_PLAN_H_
#define PE_FIT_PLAN_H_

#include <algorithm>

#include "pe_domain_map.h"

namespace pe {

// Pairs per work unit.  A pair costs a copy of the segment plus one scan per decision, so 32 pairs already
// amortise the unit's fixed cost (the segment's ids and labels into LDS), and 2000 candidates of one rack
// still spread over 63 workgroups.
constexpr int FIT_UNIT_PAIRS = 32;
static_assert(FIT_UNIT_PAIRS >= 1 && FIT_UNIT_PAIRS <= 256, "FIT_UNIT_PAIRS");
constexpr int64_t FIT_MAX_PAIRS = 2147483646;   // n_pairs in [0, 2^31 - 1)

enum FitPlanError {
  FIT_OK = 0,
  FIT_BAD_TREE = 1,     // tree_plan_build refused the hierarchy: *tree_error says how
  FIT_BAD_LEVEL = 2,    // level outside [0, n_levels)
  FIT_BAD_COUNT = 3,    // n_pairs outside [0, 2^31 - 1) or n_jobs outside [0, 2^31 - 1]
  FIT_NO_PAIRS = 4,     // pair_job or pair_domain NULL (with n_pairs > 0)
  FIT_BAD_JOB = 5,      // a pair_job outside [0, n_jobs); index = the pair
  FIT_BAD_DOMAIN = 6    // a pair_domain outside [0, size[level]); index = the pair
};

// One work unit: places [p0, p1) of `pairs`, all of active domain `act`.
struct FitUnit {
  int32_t act, p0, p1, pad_;
};

struct FitPlan {
  int32_t level = 0;
  int32_t n_leaf = 0;      // size[0]
  int32_t n_dom = 0;       // size[level]
  std::vector<int32_t> leaf_dom, act_of, active, pair_start, pairs, unit_start;
  std::vector<FitUnit> units;

  int64_t n_active() const { return (int64_t)active.size(); }
  int64_t n_units() const { return (int64_t)units.size(); }
};

// Builds the plan.  On any error `plan` is left exactly as it was, *bad_index (if given) receives the first
// offending index (-1 where the error has none) and, for FIT_BAD_TREE, *tree_error the hierarchy's error.  A pair
// is checked job first, then domain; the first offending pair is reported.  unit_pairs: the places of a work unit,
// FIT_UNIT_PAIRS for pe_gang_fit_domains; a caller whose pairs cost more each (pe_preempt_plan.h) cuts smaller ones.
inline FitPlanError fit_plan_build(FitPlan& plan, int64_t n_jobs, int64_t n_pairs, const int32_t* pair_job,
                                   const int32_t* pair_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                                   const int32_t* parent, TreePlanError* tree_error = nullptr,
                                   int64_t* bad_index = nullptr, int unit_pairs = FIT_UNIT_PAIRS) {
  auto fail = [&](FitPlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  TreePlan tree;
  int64_t tbad = -1;
  const TreePlanError te = tree_plan_build(tree, n_levels, level_size, parent, &tbad);
  if (tree_error) *tree_error = te;
  if (te != TREE_OK) return fail(FIT_BAD_TREE, tbad);
  if (level < 0 || level >= n_levels) return fail(FIT_BAD_LEVEL, -1);
  if (n_jobs < 0 || n_jobs > (int64_t)INT32_MAX || n_pairs < 0 || n_pairs > FIT_MAX_PAIRS) return fail(FIT_BAD_COUNT, -1);
  if (n_pairs > 0 && (!pair_job || !pair_domain)) return fail(FIT_NO_PAIRS, -1);
  const int32_t n_dom = tree.size[level];
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (pair_job[p] < 0 || pair_job[p] >= n_jobs) return fail(FIT_BAD_JOB, p);
    if (pair_domain[p] < 0 || pair_domain[p] >= n_dom) return fail(FIT_BAD_DOMAIN, p);
  }
  FitPlan f;
  f.level = level;
  f.n_leaf = tree.size[0];
  f.n_dom = n_dom;
  domain_map_build(tree, parent, level, n_pairs, pair_domain, f.leaf_dom, f.act_of, f.active);
  const size_t A = f.active.size();
  csr_deal(A, n_pairs, [&](int64_t p) { return f.act_of[(size_t)pair_domain[p]]; }, nullptr, f.pair_start, f.pairs);
  // the units: each domain's range cut into runs of unit_pairs, the last one shorter
  f.unit_start.assign(A + 1, 0);
  for (size_t a = 0; a < A; ++a) {
    for (int32_t p0 = f.pair_start[a]; p0 < f.pair_start[a + 1]; p0 += unit_pairs)
      f.units.push_back(FitUnit{(int32_t)a, p0, std::min(p0 + unit_pairs, f.pair_start[a + 1]), 0});
    f.unit_start[a + 1] = (int32_t)f.units.size();
  }
  plan = std::move(f);
  if (bad_index) *bad_index = -1;
  return FIT_OK;
}

// ---- working copies for the segments too large for LDS
// A unit of a domain with more than `lds_nodes` nodes works on a private copy of the segment's four residual
// rows in global memory.  One copy per unit would grow with P, so a large domain gets k <= its units copies
// and k workgroups, workgroup s taking the domain's units s, s + k, ...  With n_large large domains among the
// shard's Ns nodes, domain a of n_a nodes gets
//   k_a = clamp(FIT_SCRATCH_MULT * Ns / (n_large * n_a), 1, units of a)
// copies.  Large domains are disjoint, so the copies hold at most
//   sum of max(n_a, FIT_SCRATCH_MULT * Ns / n_large) <= (1 + FIT_SCRATCH_MULT) * Ns
// nodes (32 B each), whatever P is.
constexpr int64_t FIT_SCRATCH_MULT = 3;

// One workgroup of the large-segment kernel: active domain `act`, units u0 + s, u0 + s + k, ... below u1, on
// the copy whose row d < 4 begins at cell at + d * n of the scratch array (n = the segment's node count).
struct FitLarge {
  int32_t act, u0, u1, k, s, pad_;
  int64_t at;
};

// The large domains' workgroups from the segment bounds seg_off[A + 1] read back from the device; returns the
// nodes of scratch they need (0: no large domain).
inline int64_t fit_scratch_layout(const FitPlan& plan, const int32_t* seg_off, int64_t Ns, int lds_nodes,
                                  std::vector<FitLarge>& out) {
  out.clear();
  const int64_t A = plan.n_active();
  int64_t n_large = 0;
  for (int64_t a = 0; a < A; ++a) n_large += seg_off[a + 1] - seg_off[a] > lds_nodes;
  int64_t at = 0;
  for (int64_t a = 0; a < A && n_large > 0; ++a) {
    const int64_t n = seg_off[a + 1] - seg_off[a];
    if (n <= lds_nodes) continue;
    const int32_t u0 = plan.unit_start[(size_t)a], u1 = plan.unit_start[(size_t)a + 1];
    const int64_t k = std::max<int64_t>(1, std::min<int64_t>(u1 - u0, FIT_SCRATCH_MULT * Ns / (n_large * n)));
    for (int64_t s = 0; s < k; ++s) {
      out.push_back(FitLarge{(int32_t)a, u0, u1, (int32_t)k, (int32_t)s, 0, at});
      at += 4 * n;
    }
  }
  return at / 4;
}

}  // namespace pe

#endif  // PE_FIT_PLAN_H_
