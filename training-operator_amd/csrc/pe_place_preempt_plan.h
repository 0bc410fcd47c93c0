// The plan of pe_place_preempt_domains: pe_place_greedy_domains' plan (pe_place_plan.h) with the victims, their
// release records (pe_preempt_plan.h) and every job's candidate list.  Plain C++, no HIP: the engine builds it on
// the host once per call, and tests/cpp/test_place_preempt_plan.cc builds it under the sanitizers.
//
// Beside the base plan it holds
//   jobs[J]              the jobs in plan order (per active domain, priority desc, index asc), each with its groups
//                        [g0, g1) and its list range [v0, v1) in the caller's job_vic, which the kernel reads as it is
//   rec_start[V + 1], recs[R]   pe_preempt_plan.h's release records, per victim
//   vic_owner[V], vic_act[V]    the level-`level` domain whose jobs list victim v and its active index, -1 = in no
//                        list.  A victim belongs to ONE workgroup: the same victim in the lists of jobs of two
//                        domains is refused (the same victim in many lists of one domain is the point of the call)
// The release bound: all the call's victims, listed or not, as ONE pe_release_gangs call against the caller's
// current residuals and reset snapshot (pe_ledger_plan.h: products and sums in 128 bits).  What passes it cannot
// cross the snapshot or wrap for any subset of the victims, whatever the jobs take in between: takes only lower a
// residual, and never below 0 in a dimension they move.
#ifndef PE_PLACE_PREEMPT_PLAN_H_
#define PE_PLACE_PREEMPT_PLAN_H_

#include "pe_ledger_plan.h"
#include "pe_place_plan.h"
#include "pe_preempt_plan.h"

namespace pe {

constexpr uint32_t PREEMPT_DRY_RUN = 1u;   // PE_PREEMPT_DRY_RUN

// One job, in plan order: its index in the caller's batch, its groups [g0, g1) and its candidate victims
// list[v0 .. v1), at most 64, in the caller's job_vic.  32 B: no record straddles a 64-B line.
struct PreemptJob {
  int32_t job, g0, g1, v0, v1, pad_[3];
};
static_assert(sizeof(PreemptJob) == 32, "PreemptJob must be 32 B");

enum PlacePreemptError {
  PP_OK = 0,
  PP_BAD_PLACE = 1,     // place_plan_build refused: *place_error (and *tree_error) say how
  PP_BAD_VICTIMS = 2,   // preempt_plan_build refused the victims or a list: *pre_error says how, in its words for a
                        // pair = a job
  PP_TWO_DOMAINS = 3,   // a victim in the lists of jobs of two domains; index = the second position in job_vic
  PP_BAD_FLAGS = 4,     // a flags bit the call does not know
  PP_OVER = 5           // the release bound: more is given back than was taken; index = the node
};

struct PlacePreemptPlan {
  PlacePlan base;
  bool dry_run = false;
  int64_t n_victims = 0;
  std::vector<PreemptJob> jobs;
  std::vector<int32_t> rec_start;
  std::vector<PreRec> recs;
  std::vector<int32_t> vic_owner, vic_act;

  int64_t n_recs() const { return (int64_t)recs.size(); }
};

// Builds the plan.  res(n) / res0(n): the four current / reset-snapshot residuals of node n; `ledger`: the scratch
// of the release bound (pe_ledger_plan.h; its node map sized by the inventory and all -1 between calls).  The checks
// run in this order: the base plan's, the victims and the lists, the two-domain rule, the flags, the release bound;
// the first offence is reported.  On any error `plan` and `ledger` are left exactly as they were and *bad_index (if
// given) receives the first offending index (-1 where the error has none).
template <class Res, class Res0>
inline PlacePreemptError place_preempt_plan_build(
    PlacePreemptPlan& plan, LedgerPlan& ledger, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
    const int32_t* group_count, const int32_t* job_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
    const int32_t* parent, int64_t n_total, int64_t n_victims, const int32_t* vic_group_off,
    const int32_t* vic_group_count, const int64_t* vic_group_req, const int32_t* vic_pod_node, const int32_t* job_vic_off,
    const int32_t* job_vic, uint32_t flags, Res res, Res0 res0, PlacePlanError* place_error = nullptr,
    TreePlanError* tree_error = nullptr, PreemptPlanError* pre_error = nullptr, int64_t* bad_index = nullptr) {
  auto fail = [&](PlacePreemptError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  PlacePreemptPlan p;
  int64_t bad = -1;
  const PlacePlanError be = place_plan_build(p.base, n_jobs, job_group_off, priority, group_count, job_domain, level,
                                             n_levels, level_size, parent, tree_error, &bad);
  if (place_error) *place_error = be;
  if (be != PLACE_OK) return fail(PP_BAD_PLACE, bad);
  // ---- the victims and the lists: the preempt call's checks and records, every job one pair (job, job_domain)
  std::vector<int32_t> self((size_t)n_jobs);
  std::iota(self.begin(), self.end(), 0);
  PreemptPlan pre;
  const PreemptPlanError ve =
      preempt_plan_build(pre, n_jobs, n_total, n_victims, vic_group_off, vic_group_count, vic_group_req, vic_pod_node,
                         n_jobs, self.data(), job_domain, job_vic_off, job_vic, level, n_levels, level_size, parent,
                         nullptr, nullptr, &bad);
  if (pre_error) *pre_error = ve;
  if (ve != PRE_OK) return fail(PP_BAD_VICTIMS, bad);
  const int64_t V = n_victims;
  p.n_victims = V;
  p.vic_owner.assign((size_t)V, -1);
  p.vic_act.assign((size_t)V, -1);
  for (int64_t j = 0; j < n_jobs; ++j)
    for (int32_t i = job_vic_off[j]; i < job_vic_off[j + 1]; ++i) {
      int32_t& owner = p.vic_owner[(size_t)job_vic[i]];
      if (owner >= 0 && owner != job_domain[j]) return fail(PP_TWO_DOMAINS, i);
      owner = job_domain[j];
    }
  for (int64_t v = 0; v < V; ++v)
    if (p.vic_owner[(size_t)v] >= 0) p.vic_act[(size_t)v] = p.base.act_of[(size_t)p.vic_owner[(size_t)v]];
  if (flags & ~PREEMPT_DRY_RUN) return fail(PP_BAD_FLAGS, -1);
  p.dry_run = (flags & PREEMPT_DRY_RUN) != 0;
  p.jobs.resize((size_t)n_jobs);
  for (int64_t i = 0; i < n_jobs; ++i) {
    const int32_t j = p.base.jobs[(size_t)i];
    p.jobs[(size_t)i] = PreemptJob{j, job_group_off[j], job_group_off[j + 1], job_vic_off[j], job_vic_off[j + 1], {0, 0, 0}};
  }
  p.rec_start = std::move(pre.rec_start);
  p.recs = std::move(pre.recs);
  // ---- the release bound, last: a ledger plan that succeeds is overwritten, and nothing can fail after it
  const LedgerPlanError le = ledger_plan_build(ledger, LEDGER_RELEASE, n_total, n_victims, vic_group_off, vic_group_count,
                                               vic_group_req, vic_pod_node, res, res0, nullptr, &bad);
  if (le != LEDGER_OK) return fail(PP_OVER, bad);   // (the gangs passed gang_slots_check above: LEDGER_OVER)
  plan = std::move(p);
  if (bad_index) *bad_index = -1;
  return PP_OK;
}

}  // namespace pe

#endif  // PE_PLACE_PREEMPT_PLAN_H_
