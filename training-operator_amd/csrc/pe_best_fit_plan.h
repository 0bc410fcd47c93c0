// The plan of pe_place_best_fit_domains: pe_place_first_fit_domains' plan (pe_first_fit_plan.h validates the
// hierarchy, the batch order and the pair list) with what the best-fit rounds of pe_place_best_fit.hip read on top.
// Plain C++, no HIP: the engine builds it on the host once per call, and tests/cpp/test_best_fit_plan.cc builds it
// under the sanitizers.
//
// A pair that names a domain which an earlier pair of the same job names already is a REPEAT: it has the slots of
// that earlier pair and a larger p, so it can never win, and it is dropped.  The pairs that stay are KEPT.
//   rank[J], leaf_dom, act_of, active, pod_off   the first-fit plan's, unchanged
//   repeat[P]            1 for a repeat, 0 for a kept pair
//   kept_start[J + 1], kept[K]   CSR from job to its kept pairs, ascending p
//   q_start[A + 1], queue[K]     CSR from active domain to its QUEUE: the (job, pair) entries that name the domain,
//                        sorted by rank[job] -- a job has at most one entry in a queue
//   ref_group[J]         the job's REFERENCE GROUP, as an index into the batch's groups: the group with the largest
//                        group_count, ties to the first; -1 for a job without pods
// Every active domain keeps at least one entry: the first pair that names it is kept.
#ifndef PE_BEST_FIT_PLAN_H_
#define PE_BEST_FIT_PLAN_H_

#include "pe_first_fit_plan.h"

namespace pe {

// One queue entry; the device's BestFitEntry (pe_kernels.h) has the same two words.
struct BestFitCand {
  int32_t job, pair;
};

struct BestFitPlan {
  int32_t level = 0;
  int32_t n_leaf = 0;      // size[0]
  int32_t n_dom = 0;       // size[level]
  std::vector<int32_t> leaf_dom, act_of, active, rank, kept_start, kept, q_start, ref_group;
  std::vector<uint8_t> repeat;
  std::vector<BestFitCand> queue;
  std::vector<int64_t> pod_off;

  int64_t n_active() const { return (int64_t)active.size(); }
  int64_t n_kept() const { return (int64_t)kept.size(); }
  int64_t pods() const { return pod_off.empty() ? 0 : pod_off.back(); }
};

// Builds the plan.  The errors, their order and *bad_index / *tree_error are first_fit_plan_build's.  On any error
// `plan` is left exactly as it was.
inline FitPlanError best_fit_plan_build(BestFitPlan& plan, int64_t n_jobs, const int32_t* job_group_off,
                                        const int32_t* priority, const int32_t* group_count, int64_t n_pairs,
                                        const int32_t* pair_job, const int32_t* pair_domain, int32_t level,
                                        int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                        TreePlanError* tree_error = nullptr, int64_t* bad_index = nullptr) {
  FirstFitPlan ff;
  const FitPlanError err = first_fit_plan_build(ff, n_jobs, job_group_off, priority, group_count, n_pairs, pair_job,
                                                pair_domain, level, n_levels, level_size, parent, tree_error, bad_index);
  if (err != FIT_OK) return err;
  BestFitPlan p;
  p.level = ff.level;
  p.n_leaf = ff.n_leaf;
  p.n_dom = ff.n_dom;
  const size_t A = ff.active.size();
  // the repeats: a job's candidates in ascending p, each domain stamped with the job that named it last
  p.repeat.assign((size_t)n_pairs, 0);
  p.kept_start.assign((size_t)n_jobs + 1, 0);
  p.kept.reserve((size_t)n_pairs);
  std::vector<int32_t> named(A, -1);
  for (int64_t j = 0; j < n_jobs; ++j) {
    for (int32_t c = ff.cand_start[(size_t)j]; c < ff.cand_start[(size_t)j + 1]; ++c) {
      const int32_t q = ff.cand[(size_t)c];
      int32_t& by = named[(size_t)ff.act_of[(size_t)pair_domain[q]]];
      if (by == (int32_t)j) {
        p.repeat[(size_t)q] = 1;
      } else {
        by = (int32_t)j;
        p.kept.push_back(q);
      }
    }
    p.kept_start[(size_t)j + 1] = (int32_t)p.kept.size();
  }
  // the queues: the first-fit queues, sorted by (rank, k), without the repeats
  p.q_start.assign(A + 1, 0);
  p.queue.reserve(p.kept.size());
  for (size_t a = 0; a < A; ++a) {
    for (int32_t i = ff.q_start[a]; i < ff.q_start[a + 1]; ++i) {
      const FirstFitCand& e = ff.queue[(size_t)i];
      if (!p.repeat[(size_t)e.pair]) p.queue.push_back(BestFitCand{e.job, e.pair});
    }
    p.q_start[a + 1] = (int32_t)p.queue.size();
  }
  p.ref_group.assign((size_t)n_jobs, -1);
  for (int64_t j = 0; j < n_jobs; ++j) {
    int32_t most = 0;
    for (int32_t g = job_group_off[j]; g < job_group_off[j + 1]; ++g)
      if (group_count[g] > most) {
        most = group_count[g];
        p.ref_group[(size_t)j] = g;
      }
  }
  p.leaf_dom = std::move(ff.leaf_dom);
  p.act_of = std::move(ff.act_of);
  p.active = std::move(ff.active);
  p.rank = std::move(ff.rank);
  p.pod_off = std::move(ff.pod_off);
  plan = std::move(p);
  return FIT_OK;
}

}  // namespace pe

#endif  // PE_BEST_FIT_PLAN_H_
