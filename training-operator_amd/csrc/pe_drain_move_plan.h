// The plan of pe_drain_move_domains: pe_drain_fit_domains' plan (pe_drain_plan.h) -- every check and every product
// unchanged: the slot list, the runs, the active domains and, per active domain, its candidates in ascending c
// (fit.pair_start / fit.pairs; the work units are not used: one workgroup owns a domain) -- then the flags, then
// the release bound.  Plain C++, no HIP: the engine builds it on the host once per call, and
// tests/cpp/test_drain_move_plan.cc builds it under the sanitizers.
//
// The release bound: ALL the candidates' evicted slots, of candidates that will fit or not, as ONE
// pe_release_gangs call against the caller's current residuals and reset snapshot (pe_ledger_plan.h: products and
// sums in 128 bits).  The evicted slots are handed to it as one gang whose groups are the runs, every slot of a run
// naming the candidate's node.  The candidates are cordoned, so no take of the call touches a node that is given
// back to: what passes the bound cannot cross the snapshot or wrap for any subset of the candidates.
#ifndef PE_DRAIN_MOVE_PLAN_H_
#define PE_DRAIN_MOVE_PLAN_H_

#include "pe_drain_plan.h"
#include "pe_ledger_plan.h"

namespace pe {

constexpr uint32_t DRAIN_DRY_RUN = 1u;   // PE_DRAIN_DRY_RUN

enum DrainMoveError {
  DM_OK = 0,
  DM_BAD_DRAIN = 1,   // drain_plan_build refused: *drain_error (and its three companions) say how
  DM_BAD_FLAGS = 2,   // a flags bit the call does not know
  DM_OVER = 3         // the release bound: more is given back than was taken; index = the node
};

// What the call adds to the DrainPlan it is built beside.
struct DrainMovePlan {
  bool dry_run = false;
};

// Builds the plan.  removed(n): whether node n is a removed slot; res(n) / res0(n): the four current / reset-snapshot
// residuals of node n; `ledger`: the scratch of the release bound (its node map sized by the inventory and all -1
// between calls).  The checks run in this order: drain_plan_build's, the flags, the release bound; the first offence
// is reported.  On any error `drain`, `plan` and `ledger` are left exactly as they were and *bad_index (if given) receives
// the first offending index (-1 where the error has none).
template <class Removed, class Res, class Res0>
inline DrainMoveError drain_move_plan_build(DrainPlan& drain, DrainMovePlan& plan, LedgerPlan& ledger, int64_t n_total,
                                            int64_t n_gangs, const int32_t* group_off, const int32_t* group_count,
                                            const int64_t* group_req, const int32_t* pod_node, int64_t n_cands,
                                            const int32_t* cand_node, const int32_t* cand_domain, int32_t level,
                                            int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                            uint32_t flags, Removed removed, Res res, Res0 res0,
                                            DrainPlanError* drain_error = nullptr, GangSlotsError* gangs_error = nullptr,
                                            FitPlanError* fit_error = nullptr, TreePlanError* tree_error = nullptr,
                                            int64_t* bad_index = nullptr) {
  auto fail = [&](DrainMoveError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  int64_t bad = -1;
  // built aside, on the caller's node map (the one map, all -1 between calls, that drain_plan_build keeps so)
  DrainPlan built;
  built.cand_of.swap(drain.cand_of);
  const DrainPlanError de =
      drain_plan_build(built, n_total, n_gangs, group_off, group_count, group_req, pod_node, n_cands, cand_node,
                       cand_domain, level, n_levels, level_size, parent, removed, gangs_error, fit_error, tree_error, &bad);
  drain.cand_of.swap(built.cand_of);
  if (drain_error) *drain_error = de;
  if (de != DRAIN_OK) return fail(DM_BAD_DRAIN, bad);
  if (flags & ~DRAIN_DRY_RUN) return fail(DM_BAD_FLAGS, -1);
  // ---- the release bound: one gang, its groups the runs, every slot of candidate c's runs on cand_node[c]
  const DrainPlan& d = built;
  const int64_t C = n_cands, R = d.n_runs(), E = d.n_evicted();
  std::vector<int32_t> counts((size_t)R), nodes((size_t)E);
  std::vector<int64_t> reqs((size_t)R * 4);
  for (int64_t c = 0; c < C; ++c) {
    for (int32_t r = d.run_start[(size_t)c]; r < d.run_start[(size_t)c + 1]; ++r) {
      counts[(size_t)r] = d.runs[(size_t)r].count;
      for (int k = 0; k < 4; ++k) reqs[(size_t)r * 4 + k] = group_req[(int64_t)d.runs[(size_t)r].group * 4 + k];
    }
    std::fill(nodes.begin() + d.slot_start[(size_t)c], nodes.begin() + d.slot_start[(size_t)c + 1], cand_node[c]);
  }
  const int32_t one_gang[2] = {0, (int32_t)R};   // R <= E <= 2^31 - 1
  const LedgerPlanError le = ledger_plan_build(ledger, LEDGER_RELEASE, n_total, 1, one_gang, counts.data(), reqs.data(),
                                               nodes.data(), res, res0, nullptr, &bad);
  if (le != LEDGER_OK) return fail(DM_OVER, bad);   // (the runs passed gang_slots_check in the book: LEDGER_OVER)
  built.cand_of.swap(drain.cand_of);
  drain = std::move(built);
  plan.dry_run = (flags & DRAIN_DRY_RUN) != 0;
  if (bad_index) *bad_index = -1;
  return DM_OK;
}

}  // namespace pe

#endif  // PE_DRAIN_MOVE_PLAN_H_
