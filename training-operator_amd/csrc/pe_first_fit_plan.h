// The plan of pe_place_first_fit_domains: the caller's hierarchy, batch order and (job, domain) pair list
// validated and turned into what the round kernel of pe_place.hip reads.  Plain C++, no HIP: the engine builds it
// on the host once per call, and tests/cpp/test_first_fit_plan.cc builds it under the sanitizers.
//
// The hierarchy and the pairs are pe_gang_fit_domains' (fit_plan_build validates them, and the leaf map and the
// ACTIVE domains -- those named by some pair -- are its).  On top of them the plan holds
//   rank[J]              job j's place in the (priority desc, index asc) order
//   cand_start[J + 1], cand[P]   CSR from job to its candidates, ascending p: cand[cand_start[j] + k] is the pair
//                        at position k of job j's list
//   q_start[A + 1], queue[P]     CSR from active domain to its QUEUE: the (job, k, pair, last) entries that name
//                        the domain, sorted by (rank[job], k); last = 1 on a job's last candidate
//   pod_off[G + 1]       each group's first pod slot (groups in input order)
// The batch arrays (offsets monotonic, counts >= 0) are the engine's to check before the plan is built.
#ifndef PE_FIRST_FIT_PLAN_H_
#define PE_FIRST_FIT_PLAN_H_

#include "pe_fit_plan.h"

namespace pe {

// One queue entry; the device's FirstFitEntry (pe_kernels.h) has the same four words.
struct FirstFitCand {
  int32_t job, k, pair, last;
};

struct FirstFitPlan {
  int32_t level = 0;
  int32_t n_leaf = 0;      // size[0]
  int32_t n_dom = 0;       // size[level]
  std::vector<int32_t> leaf_dom, act_of, active, rank, cand_start, cand, q_start;
  std::vector<FirstFitCand> queue;
  std::vector<int64_t> pod_off;

  int64_t n_active() const { return (int64_t)active.size(); }
  int64_t pods() const { return pod_off.empty() ? 0 : pod_off.back(); }
};

// Builds the plan.  The errors, their order and *bad_index / *tree_error are fit_plan_build's.  On any error
// `plan` is left exactly as it was.  priority may be NULL only with n_jobs == 0.
inline FitPlanError first_fit_plan_build(FirstFitPlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                         const int32_t* priority, const int32_t* group_count, int64_t n_pairs,
                                         const int32_t* pair_job, const int32_t* pair_domain, int32_t level,
                                         int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                         TreePlanError* tree_error = nullptr, int64_t* bad_index = nullptr) {
  FitPlan fit;
  const FitPlanError err =
      fit_plan_build(fit, n_jobs, n_pairs, pair_job, pair_domain, level, n_levels, level_size, parent, tree_error, bad_index);
  if (err != FIT_OK) return err;
  FirstFitPlan p;
  p.level = fit.level;
  p.n_leaf = fit.n_leaf;
  p.n_dom = fit.n_dom;
  p.leaf_dom = std::move(fit.leaf_dom);
  p.act_of = std::move(fit.act_of);
  p.active = std::move(fit.active);
  // jobs by (priority desc, index asc)
  std::vector<int32_t> order((size_t)n_jobs);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [priority](int32_t a, int32_t b) { return priority[a] > priority[b]; });
  p.rank.resize((size_t)n_jobs);
  for (int64_t i = 0; i < n_jobs; ++i) p.rank[(size_t)order[(size_t)i]] = (int32_t)i;
  // every job's candidates in ascending p; then the queues: the entries dealt to their domains job by job in rank
  // order, candidate by candidate, so every queue comes out sorted by (rank, k); fit's pair_start holds the bounds
  csr_deal((size_t)n_jobs, n_pairs, [&](int64_t q) { return pair_job[q]; }, nullptr, p.cand_start, p.cand);
  p.q_start = std::move(fit.pair_start);
  std::vector<int32_t> fill(p.q_start.begin(), p.q_start.end() - 1);
  p.queue.resize((size_t)n_pairs);
  for (int32_t j : order) {
    const int32_t c0 = p.cand_start[(size_t)j], c1 = p.cand_start[(size_t)j + 1];
    for (int32_t c = c0; c < c1; ++c) {
      const int32_t q = p.cand[(size_t)c];
      p.queue[(size_t)fill[(size_t)p.act_of[(size_t)pair_domain[q]]]++] = FirstFitCand{j, c - c0, q, c + 1 == c1};
    }
  }
  p.pod_off = pod_offsets(n_jobs > 0 ? job_group_off[n_jobs] : 0, group_count);
  plan = std::move(p);
  return FIT_OK;
}

}  // namespace pe

#endif  // PE_FIRST_FIT_PLAN_H_
