// The plan of pe_release_gangs / pe_assume_gangs: the caller's gangs validated (pe_gang_slots.h) and turned into the
// new ABSOLUTE residuals of every node they touch.  Plain C++, no HIP: the engine builds it on the host once per
// call against its mirror, and tests/cpp/test_ledger_plan.cc builds it under the sanitizers.
//
// One pass over the pod slots in input order.  Every run of one node inside a group is one STEP (node, run length x
// request, the product formed in 128 bits).  A node is looked up once, when its first step arrives: its current
// residuals are copied from the mirror into the scratch list `touched`, and `place` remembers where.  A step is
// applied to that scratch entry, release adding and assume subtracting, and the bound is checked as it is applied,
// in the dimensions the step moves:
//   release   scratch <= the reset snapshot   ("more is given back than was taken")
//   assume    scratch >= 0                    ("the pods do not fit")
// Both operations are monotone in every dimension, so a step crosses the bound exactly when the call's totals on
// the node do, and the first crossing in slot order names the node.  A dimension no step moves is never looked at:
// cap - used may be negative.  Every value that is stored passed its bound, so the scratch stays within int64.
// Steps on a removed slot (residual[0] == LEDGER_REMOVED) count nothing, as slots holding -1.
#ifndef PE_LEDGER_PLAN_H_
#define PE_LEDGER_PLAN_H_

#include <vector>

#include "pe_gang_slots.h"

namespace pe {

constexpr int64_t LEDGER_REMOVED = INT64_MIN;   // pe_kernels.h NEVER: the residual of a removed slot

enum LedgerOp { LEDGER_RELEASE = 0, LEDGER_ASSUME = 1 };

enum LedgerPlanError {
  LEDGER_OK = 0,
  LEDGER_BAD_GANGS = 1,   // gang_slots_check refused the gangs: *gangs_error says how, index = its index
  LEDGER_OVER = 2,        // release: more is given back than was taken; index = the node
  LEDGER_UNDER = 3        // assume: the pods do not fit; index = the node
};

// A touched node and its residuals after the call: the greedy's update record {node (i64), res[4]} with the GLOBAL
// id (the engine ships it with the shard's local index).
struct LedgerUpd {
  int64_t node;
  int64_t res[4];
};
static_assert(sizeof(LedgerUpd) == 40, "LedgerUpd must be 40 B");

struct LedgerPlan {
  std::vector<int32_t> place;       // node -> its index in the call's scratch list; all -1 between calls
  std::vector<LedgerUpd> touched;   // the last successful call's touched nodes, in the order of their first step
  int64_t pods = 0;                 // ... its pod slots that counted
  int64_t steps = 0;                // ... and its steps
};

// Builds the plan of one call.  res(n) / res0(n) return the four current / reset-snapshot residuals of node n (const
// int64_t*).  On any error `plan` is left exactly as it was (place all -1, touched, pods and steps of the last
// success) and *bad_index (if given) receives the offending index or node.
template <class Res, class Res0>
inline LedgerPlanError ledger_plan_build(LedgerPlan& plan, LedgerOp op, int64_t n_total, int64_t n_gangs,
                                         const int32_t* group_off, const int32_t* group_count,
                                         const int64_t* group_req, const int32_t* pod_node, Res res, Res0 res0,
                                         GangSlotsError* gangs_error = nullptr, int64_t* bad_index = nullptr) {
  int64_t slots = 0, bad = -1;
  const GangSlotsError ge =
      gang_slots_check(n_gangs, group_off, group_count, group_req, pod_node, n_total, &slots, &bad);
  if (gangs_error) *gangs_error = ge;
  if (bad_index) *bad_index = bad;
  if (ge != GANGS_OK) return LEDGER_BAD_GANGS;
  if ((int64_t)plan.place.size() != n_total) plan.place.assign((size_t)n_total, -1);
  std::vector<LedgerUpd> scratch;
  int64_t pods = 0, steps = 0, crossed = -1;
  int64_t s = 0;
  for (int64_t v = 0; v < n_gangs && crossed < 0; ++v)
    for (int32_t g = group_off[v]; g < group_off[v + 1] && crossed < 0; ++g) {
      const int64_t* const q = group_req + (int64_t)g * 4;
      gang_group_runs(pod_node, s, group_count[g], [&](int32_t node, int64_t run) {
        int32_t at = plan.place[(size_t)node];
        if (at < 0) {
          const int64_t* const now = res(node);
          if (now[0] == LEDGER_REMOVED) return true;   // (looked up again by a later step: a removed slot is rare)
          at = plan.place[(size_t)node] = (int32_t)scratch.size();
          scratch.push_back(LedgerUpd{node, {now[0], now[1], now[2], now[3]}});
        }
        LedgerUpd& u = scratch[(size_t)at];
        for (int d = 0; d < 4; ++d) {
          if (q[d] == 0) continue;
          const __int128 step = (__int128)q[d] * run;
          if (op == LEDGER_RELEASE) {
            const __int128 to = (__int128)u.res[d] + step;
            if (to > (__int128)res0(node)[d]) {
              crossed = node;
              return false;
            }
            u.res[d] = (int64_t)to;
          } else {
            const __int128 to = (__int128)u.res[d] - step;
            if (to < 0) {
              crossed = node;
              return false;
            }
            u.res[d] = (int64_t)to;
          }
        }
        pods += run;
        ++steps;
        return true;
      });
    }
  for (const LedgerUpd& u : scratch) plan.place[(size_t)u.node] = -1;
  if (crossed >= 0) {
    if (bad_index) *bad_index = crossed;
    return op == LEDGER_RELEASE ? LEDGER_OVER : LEDGER_UNDER;
  }
  plan.touched = std::move(scratch);
  plan.pods = pods;
  plan.steps = steps;
  return LEDGER_OK;
}

}  // namespace pe

#endif  // PE_LEDGER_PLAN_H_
