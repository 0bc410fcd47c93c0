// The plan of pe_drain_fit_domains: the caller's book of placed gangs (pe_gang_slots.h), its candidate nodes and
// its hierarchy validated and turned into what the kernels of pe_drain.hip read.  Plain C++, no HIP: the engine
// builds it on the host once per call, and tests/cpp/test_drain_plan.cc builds it under the sanitizers.
//
// Candidate c drains node cand_node[c] into the level-`level` domain cand_domain[c].  Its EVICTED slots are the
// pod slots s with pod_node[s] == cand_node[c], in ascending s; a candidate whose node is a removed slot evicts
// nothing (the ledger's rule).  One pass over the slots through a dense node -> candidate map counts them, a
// second one deals them (a counting sort by candidate) and cuts them into RUNS:
//   slot_start[C + 1], slot_list[E]   candidate c's evicted slots, ascending
//   run_start[C + 1], runs[R]         its runs: consecutive entries of its slot list that belong to one group --
//                                     `count` pods of group `group`, the first at place `pod0` of slot_list
// A group's slots are consecutive in the book, so a group has at most one run per candidate.  The runs of a
// candidate, in order, are the groups of ONE synthetic job, and with pair_job = c and pair_domain = cand_domain[c]
// the rest is the fit call's plan unchanged (pe_fit_plan.h fit_plan_build): active domains, the pair CSR, units of
// FIT_UNIT_PAIRS candidates, the large-segment scratch layout.  Every check of this file runs before it.
#ifndef PE_DRAIN_PLAN_H_
#define PE_DRAIN_PLAN_H_

#include "pe_fit_plan.h"
#include "pe_gang_slots.h"

namespace pe {

constexpr int64_t DRAIN_MAX_CANDS = FIT_MAX_PAIRS;   // n_cands in [0, 2^31 - 1)

enum DrainPlanError {
  DRAIN_OK = 0,
  DRAIN_BAD_GANGS = 1,    // gang_slots_check refused the book: *gangs_error says how, index = its index
  DRAIN_BAD_SLOTS = 2,    // more than 2^31 - 1 pod slots: a slot index would not fit the slot list
  DRAIN_BAD_COUNT = 3,    // n_cands outside [0, 2^31 - 1)
  DRAIN_NO_CANDS = 4,     // cand_node or cand_domain NULL (with n_cands > 0)
  DRAIN_BAD_NODE = 5,     // a cand_node outside [0, n_total); index = the candidate
  DRAIN_DUP_NODE = 6,     // a node named by two candidates; index = the second one
  DRAIN_BAD_FIT = 7       // fit_plan_build refused the hierarchy, level or a cand_domain: *fit_error, *tree_error
};

// One run: `count` >= 1 pods of the caller's group `group`, the evicted slots slot_list[pod0 .. pod0 + count).
struct DrainRun {
  int32_t group, count;
  int64_t pod0;
};

struct DrainPlan {
  FitPlan fit;                        // pair p = candidate p
  int64_t slots = 0;                  // S: the pod slots of the book
  std::vector<int32_t> cand_of;       // node -> candidate; all -1 between calls
  std::vector<int64_t> slot_start;    // [C + 1]
  std::vector<int32_t> slot_list;     // [E]
  std::vector<int32_t> run_start;     // [C + 1]
  std::vector<DrainRun> runs;         // [R]

  int64_t n_cands() const { return slot_start.empty() ? 0 : (int64_t)slot_start.size() - 1; }
  int64_t n_evicted() const { return (int64_t)slot_list.size(); }
  int64_t n_runs() const { return (int64_t)runs.size(); }
};

// Builds the plan.  removed(n): whether node n is a removed slot.  On any error `plan` is left exactly as it was
// (cand_of all -1, the rest the last success') and *bad_index (if given) receives the first offending index (-1
// where the error has none).  Order of the checks: the book, its slot total, n_cands, the two pointers, every
// cand_node (range, then repetition, candidate by candidate), then fit_plan_build's (hierarchy, level, cand_domain).
template <class Removed>
inline DrainPlanError drain_plan_build(DrainPlan& plan, int64_t n_total, int64_t n_gangs, const int32_t* group_off,
                                       const int32_t* group_count, const int64_t* group_req, const int32_t* pod_node,
                                       int64_t n_cands, const int32_t* cand_node, const int32_t* cand_domain,
                                       int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                       Removed removed, GangSlotsError* gangs_error = nullptr,
                                       FitPlanError* fit_error = nullptr, TreePlanError* tree_error = nullptr,
                                       int64_t* bad_index = nullptr) {
  auto fail = [&](DrainPlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  int64_t S = 0, bad = -1;
  const GangSlotsError ge = gang_slots_check(n_gangs, group_off, group_count, group_req, pod_node, n_total, &S, &bad);
  if (gangs_error) *gangs_error = ge;
  if (ge != GANGS_OK) return fail(DRAIN_BAD_GANGS, bad);
  if (S > (int64_t)INT32_MAX) return fail(DRAIN_BAD_SLOTS, -1);
  if (n_cands < 0 || n_cands > DRAIN_MAX_CANDS) return fail(DRAIN_BAD_COUNT, -1);
  if (n_cands > 0 && (!cand_node || !cand_domain)) return fail(DRAIN_NO_CANDS, -1);
  const int64_t C = n_cands;
  for (int64_t c = 0; c < C; ++c)
    if (cand_node[c] < 0 || cand_node[c] >= n_total) return fail(DRAIN_BAD_NODE, c);
  if ((int64_t)plan.cand_of.size() != n_total) plan.cand_of.assign((size_t)n_total, -1);
  std::vector<int32_t>& cand_of = plan.cand_of;
  auto wipe = [&](int64_t upto) {
    for (int64_t c = 0; c < upto; ++c) cand_of[(size_t)cand_node[c]] = -1;
  };
  for (int64_t c = 0; c < C; ++c) {
    int32_t& at = cand_of[(size_t)cand_node[c]];
    if (at >= 0) {
      wipe(c);
      return fail(DRAIN_DUP_NODE, c);
    }
    at = (int32_t)c;
  }
  // the rest of the checks: the fit call's, with candidate c as pair c of job c
  FitPlan fit;
  {
    std::vector<int32_t> pair_job((size_t)C);
    std::iota(pair_job.begin(), pair_job.end(), 0);
    TreePlanError te = TREE_OK;
    const FitPlanError fe =
        fit_plan_build(fit, C, C, pair_job.data(), cand_domain, level, n_levels, level_size, parent, &te, &bad);
    if (fit_error) *fit_error = fe;
    if (tree_error) *tree_error = te;
    if (fe != FIT_OK) {
      wipe(C);
      return fail(DRAIN_BAD_FIT, bad);
    }
  }
  // a removed candidate evicts nothing: it leaves the map before the slots are looked at
  for (int64_t c = 0; c < C; ++c)
    if (removed(cand_node[c])) cand_of[(size_t)cand_node[c]] = -1;
  // ---- pass 1: evicted slots and runs per candidate.  last[c] = the group of c's latest evicted slot
  std::vector<int64_t> slot_start((size_t)C + 1, 0);
  std::vector<int32_t> run_start((size_t)C + 1, 0), last((size_t)C, -1);
  const int64_t VG = n_gangs > 0 ? group_off[n_gangs] : 0;
  int64_t s = 0;
  for (int64_t g = 0; g < VG; ++g)
    for (const int64_t e = s + group_count[g]; s < e; ++s) {
      const int32_t c = pod_node[s] >= 0 ? cand_of[(size_t)pod_node[s]] : -1;
      if (c < 0) continue;
      ++slot_start[(size_t)c + 1];
      if (last[(size_t)c] != (int32_t)g) {
        last[(size_t)c] = (int32_t)g;
        ++run_start[(size_t)c + 1];
      }
    }
  for (int64_t c = 0; c < C; ++c) {
    slot_start[(size_t)c + 1] += slot_start[(size_t)c];
    run_start[(size_t)c + 1] += run_start[(size_t)c];
  }
  // ---- pass 2: the deal.  fill[c] / rfill[c] = the next free place of c's slot list / run list
  std::vector<int32_t> slot_list((size_t)slot_start[(size_t)C]);
  std::vector<DrainRun> runs((size_t)run_start[(size_t)C]);
  std::vector<int64_t> fill(slot_start.begin(), slot_start.end() - 1);
  std::vector<int32_t> rfill(run_start.begin(), run_start.end() - 1);
  std::fill(last.begin(), last.end(), -1);
  s = 0;
  for (int64_t g = 0; g < VG; ++g)
    for (const int64_t e = s + group_count[g]; s < e; ++s) {
      const int32_t c = pod_node[s] >= 0 ? cand_of[(size_t)pod_node[s]] : -1;
      if (c < 0) continue;
      if (last[(size_t)c] != (int32_t)g) {
        last[(size_t)c] = (int32_t)g;
        runs[(size_t)rfill[(size_t)c]++] = DrainRun{(int32_t)g, 0, fill[(size_t)c]};
      }
      ++runs[(size_t)rfill[(size_t)c] - 1].count;
      slot_list[(size_t)fill[(size_t)c]++] = (int32_t)s;
    }
  wipe(C);
  plan.fit = std::move(fit);
  plan.slots = S;
  plan.slot_start = std::move(slot_start);
  plan.slot_list = std::move(slot_list);
  plan.run_start = std::move(run_start);
  plan.runs = std::move(runs);
  if (bad_index) *bad_index = -1;
  return DRAIN_OK;
}

}  // namespace pe

#endif  // PE_DRAIN_PLAN_H_
