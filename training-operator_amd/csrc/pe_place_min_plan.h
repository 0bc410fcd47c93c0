// The plan of pe_place_min_member_domains: pe_place_greedy_domains' plan (pe_place_plan.h) plus every group's
// mandatory and optional share under the job's MinMember.  Plain C++, no HIP: the engine builds it on the host
// once per call, and tests/cpp/test_place_min_plan.cc builds it under the sanitizers.
//
// For job j with pod total T_j and M_j = T_j (min_member NULL or PE_MIN_MEMBER_ALL) or min_member[j], and b_g the
// pods of the job's groups before group g:
//   mand[g] = clamp(M_j - b_g, 0, count_g), raised to count_g when it is > 0 and the group is an island group
//   opt[g]  = count_g - mand[g]
// The mandatory pods of a job are the first pods of its slot range (every group before the cut is mandatory in
// full), so they are numbered a second time without the optional ones:
//   mand_pod0[g]  the group's first MANDATORY slot, counting mandatory pods only, over all groups in input order
//   opt_pod0[g]   the group's first optional slot among ALL slots: pod_off[g] + mand[g]
//   job_shift[j]  pod_off[first group of j] - mand_pod0[first group of j]: a mandatory slot plus the shift is the
//                 pod's slot among all slots
//   job_gm[j]     one past the job's last group with mand > 0 (the job's first group when it has none): phase 1
//                 is the existing all-or-nothing loop over the records [g0, gm) with counts mand and slots
//                 mand_pod0, its log in the mandatory numbering, its pod stores shifted by job_shift
//   job_pods[j]   T_j
// The batch arrays (offsets monotonic, counts >= 0) are the engine's to check before the plan is built.
#ifndef PE_PLACE_MIN_PLAN_H_
#define PE_PLACE_MIN_PLAN_H_

#include "pe_place_plan.h"

namespace pe {

constexpr int32_t PLACE_MIN_ALL = -1;            // PE_MIN_MEMBER_ALL
constexpr uint32_t PLACE_MIN_ISLAND = 0x80000000u;   // PE_NEED_ISLAND

enum PlaceMinError {
  PLACE_MIN_OK = 0,
  PLACE_MIN_BASE = 1,    // place_plan_build refused: *base_error / *tree_error say how
  PLACE_MIN_BELOW = 2,   // a min_member below -1; index = the job
  PLACE_MIN_ABOVE = 3    // a min_member above the job's pod total; index = the job
};

struct PlaceMinPlan {
  PlacePlan base;
  std::vector<int32_t> mand, opt;            // [G]
  std::vector<int64_t> mand_pod0, opt_pod0;  // [G]
  std::vector<int32_t> job_gm;               // [J], by the caller's job index
  std::vector<int64_t> job_shift, job_pods;  // [J]
  int64_t mand_pods = 0;                     // the mandatory pods of the batch: the log's length in entries

  int64_t pods() const { return base.pods(); }
};

// Builds the plan.  On any error `plan` is left exactly as it was and *bad_index (if given) receives the first
// offending index (-1 where the error has none).  The base plan's checks come first, then min_member job by job.
inline PlaceMinError place_min_plan_build(PlaceMinPlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                          const int32_t* priority, const int32_t* group_count,
                                          const uint32_t* group_need, const int32_t* min_member,
                                          const int32_t* job_domain, int32_t level, int32_t n_levels,
                                          const int32_t* level_size, const int32_t* parent,
                                          PlacePlanError* base_error = nullptr, TreePlanError* tree_error = nullptr,
                                          int64_t* bad_index = nullptr) {
  PlaceMinPlan p;
  int64_t bad = -1;
  const PlacePlanError be = place_plan_build(p.base, n_jobs, job_group_off, priority, group_count, job_domain, level,
                                             n_levels, level_size, parent, tree_error, &bad);
  if (base_error) *base_error = be;
  if (be != PLACE_OK) {
    if (bad_index) *bad_index = bad;
    return PLACE_MIN_BASE;
  }
  const int64_t G = n_jobs > 0 ? job_group_off[n_jobs] : 0;
  p.mand.assign((size_t)G, 0);
  p.opt.assign((size_t)G, 0);
  p.mand_pod0.assign((size_t)G, 0);
  p.opt_pod0.assign((size_t)G, 0);
  p.job_gm.assign((size_t)n_jobs, 0);
  p.job_shift.assign((size_t)n_jobs, 0);
  p.job_pods.assign((size_t)n_jobs, 0);
  int64_t mrun = 0;   // mandatory pods so far
  for (int64_t j = 0; j < n_jobs; ++j) {
    const int32_t g0 = job_group_off[j], g1 = job_group_off[j + 1];
    const int64_t T = p.base.pod_off[(size_t)g1] - p.base.pod_off[(size_t)g0];
    const int32_t mm = min_member ? min_member[j] : PLACE_MIN_ALL;
    if (mm < PLACE_MIN_ALL || (int64_t)mm > T) {
      if (bad_index) *bad_index = j;
      return mm < PLACE_MIN_ALL ? PLACE_MIN_BELOW : PLACE_MIN_ABOVE;
    }
    const int64_t M = mm == PLACE_MIN_ALL ? T : (int64_t)mm;
    p.job_pods[(size_t)j] = T;
    p.job_shift[(size_t)j] = p.base.pod_off[(size_t)g0] - mrun;
    int32_t gm = g0;
    int64_t before = 0;   // b_g
    for (int32_t g = g0; g < g1; ++g) {
      const int64_t c = group_count[g];
      int64_t m = std::min(std::max<int64_t>(M - before, 0), c);
      if (m > 0 && group_need && (group_need[g] & PLACE_MIN_ISLAND)) m = c;
      p.mand[(size_t)g] = (int32_t)m;
      p.opt[(size_t)g] = (int32_t)(c - m);
      p.mand_pod0[(size_t)g] = mrun;
      p.opt_pod0[(size_t)g] = p.base.pod_off[(size_t)g] + m;
      if (m > 0) gm = g + 1;
      mrun += m;
      before += c;
    }
    p.job_gm[(size_t)j] = gm;
  }
  p.mand_pods = mrun;
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return PLACE_MIN_OK;
}

}  // namespace pe

#endif  // PE_PLACE_MIN_PLAN_H_
