// The plan of pe_gang_preempt_domains: the caller's hierarchy, pairs, victims and candidate lists validated and
// turned into what the kernels of pe_preempt.hip read.  Plain C++, no HIP: the engine builds it on the host once
// per call, and tests/cpp/test_preempt_plan.cc builds it under the sanitizers.
//
// The hierarchy, the active domains, the pairs' CSR and the work units are pe_fit_plan.h's (`fit`), with smaller
// units.  On top of that the plan holds
//   rec_start[V + 1], recs[R]   CSR from victim to its RELEASE RECORDS: one record per run of pod slots of one
//                        group on one node -- the node and request x run length, what the node gets back when the
//                        victim goes.  Slots holding -1 end a run and give no record.  A product that overflows
//                        int64 saturates at INT64_MAX; the per-node sums below then saturate too, and the
//                        engine's guard refuses the call unless the node is a removed slot (which no segment holds)
//   list_start[P + 1], list[]   the pairs' candidate victims, by PLACE of the plan's pair list (fit.pairs), each
//                        list in the caller's eviction order
//   sum_node[S], sum_q[S][4]    per node named by some record, ascending: the sum of ALL the call's records on it,
//                        saturating at UINT64_MAX -- the engine checks residual + sum <= INT64_MAX against its
//                        mirror, so that no set of releases can overflow on the device
#ifndef PE_PREEMPT_PLAN_H_
#define PE_PREEMPT_PLAN_H_

#include "pe_fit_plan.h"
#include "pe_gang_slots.h"

namespace pe {

// Pairs per work unit.  A pair of pe_gang_fit_domains is one judgement; a pair here is up to 2 K + 1 of them (K
// candidate victims, 33 at the 16 of a typical call, 129 at the limit), each a copy of the segment, the releases
// and one scan per decision.  Four pairs are already the work of a full unit of the fit call, so the unit's fixed
// cost (ids and labels into LDS) is amortised as well, and a rack that 100 gangs contest still spreads over 25
// workgroups.
constexpr int PRE_UNIT_PAIRS = 4;
static_assert(PRE_UNIT_PAIRS >= 1 && PRE_UNIT_PAIRS <= FIT_UNIT_PAIRS, "PRE_UNIT_PAIRS");
constexpr int PRE_MAX_VICTIMS = 64;   // PE_MAX_PAIR_VICTIMS: a pair's list is one 64-bit mask

enum PreemptPlanError {
  PRE_OK = 0,
  PRE_BAD_FIT = 1,          // fit_plan_build refused the hierarchy or the pairs: *fit_error, *tree_error say how
  PRE_BAD_VICTIMS = 2,      // n_victims outside [0, 2^31 - 1]
  PRE_NO_VIC_OFF = 3,       // vic_group_off NULL (n_victims > 0)
  PRE_BAD_VIC_OFF = 4,      // vic_group_off does not rise from 0; index = the offset
  PRE_NO_VIC_GROUPS = 5,    // vic_group_count or vic_group_req NULL with groups
  PRE_BAD_VIC_COUNT = 6,    // a negative count; index = the group
  PRE_BAD_VIC_REQ = 7,      // a negative request; index = the group
  PRE_NO_POD_NODE = 8,      // vic_pod_node NULL although some group has pods
  PRE_BAD_POD_NODE = 9,     // a vic_pod_node outside [-1, n_total); index = the pod slot
  PRE_TOO_MANY = 10,        // more than 2^31 - 1 release records
  PRE_NO_LIST_OFF = 11,     // pair_vic_off NULL (n_pairs > 0)
  PRE_BAD_LIST_OFF = 12,    // pair_vic_off does not rise from 0; index = the offset
  PRE_LONG_LIST = 13,       // a list longer than PRE_MAX_VICTIMS; index = the pair
  PRE_NO_LIST = 14,         // pair_vic NULL with a non-empty list
  PRE_BAD_LIST_VICTIM = 15, // a pair_vic outside [0, n_victims); index = the position in pair_vic
  PRE_DUP_VICTIM = 16       // the same victim twice in one pair's list; index = the second position in pair_vic
};
static_assert(PRE_BAD_VICTIMS - GANGS_BAD_COUNT == PRE_BAD_POD_NODE - GANGS_BAD_POD_NODE &&
                  PRE_NO_VIC_GROUPS - GANGS_NO_GROUPS == PRE_BAD_VICTIMS - GANGS_BAD_COUNT,
              "the victims' errors are pe_gang_slots.h's, shifted");

// One release record: node `node` gets q back.  sat (host only): bit d = q[d] is a saturated product.
struct PreRec {
  int64_t q[4];
  int32_t node, sat;
};
static_assert(sizeof(PreRec) == 40, "PreRec must be 40 B");

struct PreemptPlan {
  FitPlan fit;
  int64_t n_victims = 0;
  std::vector<int32_t> rec_start;
  std::vector<PreRec> recs;
  std::vector<int32_t> list_start, list;
  std::vector<int32_t> sum_node;
  std::vector<uint64_t> sum_q;

  int64_t n_recs() const { return (int64_t)recs.size(); }
  int64_t n_sums() const { return (int64_t)sum_node.size(); }
};

// Builds the plan.  The checks run in this order: the hierarchy, level and pairs (fit_plan_build), the victims,
// the lists; the first offence is reported.  On any error `plan` is left exactly as it was and *bad_index (if
// given) receives the first offending index (-1 where the error has none).
inline PreemptPlanError preempt_plan_build(PreemptPlan& plan, int64_t n_jobs, int64_t n_total, int64_t n_victims,
                                           const int32_t* vic_group_off, const int32_t* vic_group_count,
                                           const int64_t* vic_group_req, const int32_t* vic_pod_node, int64_t n_pairs,
                                           const int32_t* pair_job, const int32_t* pair_domain,
                                           const int32_t* pair_vic_off, const int32_t* pair_vic, int32_t level,
                                           int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                           FitPlanError* fit_error = nullptr, TreePlanError* tree_error = nullptr,
                                           int64_t* bad_index = nullptr) {
  auto fail = [&](PreemptPlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  PreemptPlan f;
  int64_t fbad = -1;
  const FitPlanError fe = fit_plan_build(f.fit, n_jobs, n_pairs, pair_job, pair_domain, level, n_levels, level_size,
                                         parent, tree_error, &fbad, PRE_UNIT_PAIRS);
  if (fit_error) *fit_error = fe;
  if (fe != FIT_OK) return fail(PRE_BAD_FIT, fbad);
  // ---- the victims (pe_gang_slots.h: PRE_BAD_VICTIMS .. PRE_BAD_POD_NODE are its errors, in its order)
  int64_t slots = 0, vbad = -1;
  const GangSlotsError ve = gang_slots_check(n_victims, vic_group_off, vic_group_count, vic_group_req, vic_pod_node,
                                             n_total, &slots, &vbad);
  if (ve != GANGS_OK) return fail((PreemptPlanError)((int)ve + (PRE_BAD_VICTIMS - GANGS_BAD_COUNT)), vbad);
  const int64_t V = n_victims;
  // ---- the lists
  const int64_t P = n_pairs;
  if (P > 0) {
    if (!pair_vic_off) return fail(PRE_NO_LIST_OFF, -1);
    if (pair_vic_off[0] != 0) return fail(PRE_BAD_LIST_OFF, 0);
    for (int64_t p = 0; p < P; ++p)
      if (pair_vic_off[p + 1] < pair_vic_off[p]) return fail(PRE_BAD_LIST_OFF, p + 1);
    for (int64_t p = 0; p < P; ++p)
      if (pair_vic_off[p + 1] - pair_vic_off[p] > PRE_MAX_VICTIMS) return fail(PRE_LONG_LIST, p);
    if (pair_vic_off[P] > 0 && !pair_vic) return fail(PRE_NO_LIST, -1);
    std::vector<int32_t> stamp((size_t)V, 0);   // the pair (+ 1) that listed the victim last
    for (int64_t p = 0; p < P; ++p)
      for (int32_t i = pair_vic_off[p]; i < pair_vic_off[p + 1]; ++i) {
        const int32_t v = pair_vic[i];
        if (v < 0 || v >= V) return fail(PRE_BAD_LIST_VICTIM, i);
        if (stamp[(size_t)v] == (int32_t)p + 1) return fail(PRE_DUP_VICTIM, i);
        stamp[(size_t)v] = (int32_t)p + 1;
      }
  }
  // ---- the release records: runs of one node inside a group merged
  f.n_victims = V;
  f.rec_start.assign((size_t)V + 1, 0);
  f.recs.reserve((size_t)std::min<int64_t>(slots, 1 << 20));
  int64_t s = 0;
  for (int64_t v = 0; v < V; ++v) {
    for (int32_t g = vic_group_off[v]; g < vic_group_off[v + 1]; ++g) {
      const bool held = gang_group_runs(vic_pod_node, s, vic_group_count[g], [&](int32_t node, int64_t run) {
        PreRec r{};
        r.node = node;
        for (int d = 0; d < 4; ++d)
          if (__builtin_mul_overflow(vic_group_req[(int64_t)g * 4 + d], run, &r.q[d])) {
            r.q[d] = INT64_MAX;
            r.sat |= 1 << d;
          }
        if (f.recs.size() >= (size_t)INT32_MAX) return false;
        f.recs.push_back(r);
        return true;
      });
      if (!held) return fail(PRE_TOO_MANY, -1);
    }
    f.rec_start[(size_t)v + 1] = (int32_t)f.recs.size();
  }
  // ---- the per-node sums, ascending node: the records' indices sorted by node, a stable radix sort of one byte
  // per pass (a comparison sort of 10^5 records costs more than all the rest of the plan)
  std::vector<uint64_t> order(f.recs.size()), other(f.recs.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = (uint64_t)(uint32_t)f.recs[k].node << 32 | k;
  for (int shift = 32; shift < 64; shift += 8) {
    size_t at[257] = {0};
    for (uint64_t key : order) ++at[(key >> shift & 255) + 1];
    if (std::find(at + 1, at + 257, order.size()) != at + 257) continue;   // one digit for all: nothing to do
    for (int b = 0; b < 256; ++b) at[b + 1] += at[b];
    for (uint64_t key : order) other[at[key >> shift & 255]++] = key;
    order.swap(other);
  }
  f.sum_node.reserve(order.size());
  f.sum_q.reserve(4 * order.size());
  for (uint64_t key : order) {
    const PreRec& r = f.recs[(size_t)(uint32_t)key];
    if (f.sum_node.empty() || f.sum_node.back() != r.node) {
      f.sum_node.push_back(r.node);
      f.sum_q.resize(f.sum_q.size() + 4, 0);
    }
    uint64_t* const sum = &f.sum_q[f.sum_q.size() - 4];
    for (int d = 0; d < 4; ++d)
      if ((r.sat >> d & 1) || __builtin_add_overflow(sum[d], (uint64_t)r.q[d], &sum[d])) sum[d] = UINT64_MAX;
  }
  // ---- the lists in plan order
  f.list_start.assign((size_t)P + 1, 0);
  for (int64_t i = 0; i < P; ++i) {
    const int32_t p = f.fit.pairs[(size_t)i];
    f.list_start[(size_t)i + 1] = f.list_start[(size_t)i] + (pair_vic_off[p + 1] - pair_vic_off[p]);
  }
  f.list.resize(P > 0 ? (size_t)pair_vic_off[P] : 0);
  for (int64_t i = 0; i < P; ++i) {
    const int32_t p = f.fit.pairs[(size_t)i];
    std::copy(pair_vic + pair_vic_off[p], pair_vic + pair_vic_off[p + 1], f.list.begin() + f.list_start[(size_t)i]);
  }
  plan = std::move(f);
  if (bad_index) *bad_index = -1;
  return PRE_OK;
}

}  // namespace pe

#endif  // PE_PREEMPT_PLAN_H_
