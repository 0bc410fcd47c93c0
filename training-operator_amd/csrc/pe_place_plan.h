// The plan of pe_place_greedy_domains: the caller's hierarchy and job -> domain assignment validated and
// turned into what the kernels of pe_place.hip read.  Plain C++, no HIP: the engine builds it on the host once
// per call, and tests/cpp/test_place_plan.cc builds it under the sanitizers.
//
// The hierarchy is pe_gang_capacity_tree's (pe_tree_plan.h validates it).  For the call's `level` the plan holds
//   leaf_dom, act_of, active[A]   pe_domain_map.h's maps; a domain is active when it has at least one job
//   job_start[A + 1], jobs[J]   CSR from active domain to its jobs in (priority desc, index asc) order
//   pod_off[G + 1]      each group's first pod slot (groups in input order)
// The batch arrays (offsets monotonic, counts >= 0) are the engine's to check before the plan is built.
#ifndef PE_PLACE_PLAN_H_
#define PE_PLACE_PLAN_H_

#include <algorithm>

#include "pe_domain_map.h"

namespace pe {

enum PlacePlanError {
  PLACE_OK = 0,
  PLACE_BAD_TREE = 1,     // tree_plan_build refused the hierarchy: *tree_error says how
  PLACE_BAD_LEVEL = 2,    // level outside [0, n_levels)
  PLACE_NO_DOMAINS = 3,   // job_domain NULL (with n_jobs > 0)
  PLACE_BAD_DOMAIN = 4    // a job_domain outside [0, size[level]); index = the job
};

struct PlacePlan {
  int32_t level = 0;
  int32_t n_leaf = 0;      // size[0]
  int32_t n_dom = 0;       // size[level]
  std::vector<int32_t> leaf_dom, act_of, active, job_start, jobs;
  std::vector<int64_t> pod_off;

  int64_t n_active() const { return (int64_t)active.size(); }
  int64_t pods() const { return pod_off.empty() ? 0 : pod_off.back(); }
};

// Builds the plan.  On any error `plan` is left exactly as it was, *bad_index (if given) receives the first
// offending index (-1 where the error has none) and, for PLACE_BAD_TREE, *tree_error the hierarchy's error.
inline PlacePlanError place_plan_build(PlacePlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                       const int32_t* priority, const int32_t* group_count, const int32_t* job_domain,
                                       int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                       TreePlanError* tree_error = nullptr, int64_t* bad_index = nullptr) {
  auto fail = [&](PlacePlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  TreePlan tree;
  int64_t tbad = -1;
  const TreePlanError te = tree_plan_build(tree, n_levels, level_size, parent, &tbad);
  if (tree_error) *tree_error = te;
  if (te != TREE_OK) return fail(PLACE_BAD_TREE, tbad);
  if (level < 0 || level >= n_levels) return fail(PLACE_BAD_LEVEL, -1);
  if (n_jobs > 0 && !job_domain) return fail(PLACE_NO_DOMAINS, -1);
  const int32_t n_dom = tree.size[level];
  for (int64_t j = 0; j < n_jobs; ++j)
    if (job_domain[j] < 0 || job_domain[j] >= n_dom) return fail(PLACE_BAD_DOMAIN, j);
  PlacePlan p;
  p.level = level;
  p.n_leaf = tree.size[0];
  p.n_dom = n_dom;
  domain_map_build(tree, parent, level, n_jobs, job_domain, p.leaf_dom, p.act_of, p.active);
  // jobs by (priority desc, index asc), then dealt to their domains in that order
  std::vector<int32_t> order((size_t)n_jobs);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [priority](int32_t a, int32_t b) { return priority[a] > priority[b]; });
  csr_deal(p.active.size(), n_jobs, [&](int64_t j) { return p.act_of[(size_t)job_domain[j]]; }, order.data(),
           p.job_start, p.jobs);
  p.pod_off = pod_offsets(n_jobs > 0 ? job_group_off[n_jobs] : 0, group_count);
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return PLACE_OK;
}

}  // namespace pe

#endif  // PE_PLACE_PLAN_H_
