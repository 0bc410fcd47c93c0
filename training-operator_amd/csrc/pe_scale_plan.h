// The plan of pe_scale_up_domains: the caller's templates, new slots, pairs and hierarchy validated and turned into
// what the kernels of pe_scale.hip read.  Plain C++, no HIP: the engine builds it on the host once per call, and
// tests/cpp/test_scale_plan.cc builds it under the sanitizers.
//
// The hierarchy, the active domains and the pairs' CSR are pe_fit_plan.h's (`fit`, fit_plan_build unchanged).  A pair
// of the fit call is one judgement; pair p here is up to kmax[p] + 1 of them, its WEIGHT, and the weights of one
// call differ by a factor of 65.  So the work units are cut by weight, not by count: a domain's CSR range is cut,
// front to back, into the longest runs whose weights add up to at most SCALE_UNIT_WEIGHT, a pair that weighs more
// on its own being a unit of one.  fit.units / fit.unit_start hold these units (the fit call's cut is replaced), so
// the large-segment layout (fit_scratch_layout) and the launches read them as they are.
//   kmax[P]   by PLACE of the plan's pair list (fit.pairs): pair_max of that pair, n_new where pair_max is NULL
#ifndef PE_SCALE_PLAN_H_
#define PE_SCALE_PLAN_H_

#include "pe_fit_plan.h"

namespace pe {

constexpr int SCALE_MAX_NEW = 64;   // PE_MAX_SCALE_NODES
// The judgements a work unit may cost: FIT_UNIT_PAIRS, the fit call's unit, which amortises the unit's fixed cost
// (the segment's ids and labels into LDS) -- with every pair_max 0 the units are exactly the fit call's.  A pair
// with pair_max >= 32 is a unit of its own, of at most SCALE_MAX_NEW + 1 = 65 judgements.  So a unit of two or more
// pairs weighs at most SCALE_UNIT_WEIGHT, no unit weighs more than 65 (about two units of the fit call), and two
// neighbouring units of one domain together weigh more than SCALE_UNIT_WEIGHT: the cut is greedy, so a domain of
// total weight W has fewer than 2 W / SCALE_UNIT_WEIGHT + 1 units.  The weight is an upper bound of the cost -- the
// attempts stop at the first that fits -- which is the safe side for the tail of a launch.
constexpr int SCALE_UNIT_WEIGHT = FIT_UNIT_PAIRS;
static_assert(SCALE_UNIT_WEIGHT >= 1, "SCALE_UNIT_WEIGHT");

enum ScalePlanError {
  SCALE_OK = 0,
  SCALE_BAD_FIT = 1,          // fit_plan_build refused the hierarchy, level or pairs: *fit_error, *tree_error say how
  SCALE_BAD_TEMPLATES = 2,    // n_templates < 0, or < 1 with pairs
  SCALE_NO_TEMPLATES = 3,     // tmpl_res NULL with templates
  SCALE_BAD_TMPL_RES = 4,     // a negative tmpl_res cell; index = the template
  SCALE_BAD_NEW = 5,          // n_new outside [0, SCALE_MAX_NEW]
  SCALE_NO_NEW = 6,           // new_slot NULL with n_new > 0
  SCALE_BAD_SLOT = 7,         // a new_slot outside [0, n_total); index = its position
  SCALE_LIVE_SLOT = 8,        // a new_slot that is not a removed slot; index = its position
  SCALE_DUP_SLOT = 9,         // a new_slot repeated; index = the second position
  SCALE_NO_PAIR_TMPL = 10,    // pair_template NULL with pairs
  SCALE_BAD_PAIR_TMPL = 11,   // a pair_template outside [0, n_templates); index = the pair
  SCALE_BAD_PAIR_MAX = 12     // a pair_max outside [0, n_new]; index = the pair
};

struct ScalePlan {
  FitPlan fit;                  // units cut by weight
  std::vector<int32_t> kmax;    // [P], in plan order
};

// The units of one CSR range [p0, p1) by weight: weight(i) of place i.  Appends to `units`.
template <class Weight>
inline void scale_cut_units(int32_t act, int32_t p0, int32_t p1, Weight weight, std::vector<FitUnit>& units) {
  int32_t u0 = p0;
  int64_t w = 0;
  for (int32_t i = p0; i < p1; ++i) {
    const int64_t wi = weight(i);
    if (i > u0 && w + wi > SCALE_UNIT_WEIGHT) {
      units.push_back(FitUnit{act, u0, i, 0});
      u0 = i;
      w = 0;
    }
    w += wi;
  }
  if (p1 > u0) units.push_back(FitUnit{act, u0, p1, 0});
}

// Builds the plan.  removed(n): whether node n is a removed slot.  The checks run in this order, and the first
// offence is reported: the hierarchy, level and pairs (fit_plan_build: tree, level, counts, pair pointers, every
// pair job first, then domain); n_templates; tmpl_res (pointer, then template by template); n_new; new_slot
// (pointer, then position by position: range, removed, repetition); pair_template (pointer, then pair by pair);
// pair_max pair by pair.  On any error `plan` is left exactly as it was and *bad_index (if given) receives the
// first offending index (-1 where the error has none).
template <class Removed>
inline ScalePlanError scale_plan_build(ScalePlan& plan, int64_t n_jobs, int64_t n_total, int32_t n_templates,
                                       const int64_t* tmpl_res, int32_t n_new, const int32_t* new_slot, int64_t n_pairs,
                                       const int32_t* pair_job, const int32_t* pair_domain,
                                       const int32_t* pair_template, const int32_t* pair_max, int32_t level,
                                       int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                       Removed removed, FitPlanError* fit_error = nullptr,
                                       TreePlanError* tree_error = nullptr, int64_t* bad_index = nullptr) {
  auto fail = [&](ScalePlanError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  ScalePlan f;
  int64_t fbad = -1;
  const FitPlanError fe =
      fit_plan_build(f.fit, n_jobs, n_pairs, pair_job, pair_domain, level, n_levels, level_size, parent, tree_error, &fbad);
  if (fit_error) *fit_error = fe;
  if (fe != FIT_OK) return fail(SCALE_BAD_FIT, fbad);
  const int64_t P = n_pairs;
  if (n_templates < 0 || (P > 0 && n_templates < 1)) return fail(SCALE_BAD_TEMPLATES, -1);
  if (n_templates > 0 && !tmpl_res) return fail(SCALE_NO_TEMPLATES, -1);
  for (int32_t t = 0; t < n_templates; ++t)
    for (int d = 0; d < 4; ++d)
      if (tmpl_res[(int64_t)t * 4 + d] < 0) return fail(SCALE_BAD_TMPL_RES, t);
  if (n_new < 0 || n_new > SCALE_MAX_NEW) return fail(SCALE_BAD_NEW, -1);
  if (n_new > 0 && !new_slot) return fail(SCALE_NO_NEW, -1);
  for (int32_t i = 0; i < n_new; ++i) {
    if (new_slot[i] < 0 || new_slot[i] >= n_total) return fail(SCALE_BAD_SLOT, i);
    if (!removed(new_slot[i])) return fail(SCALE_LIVE_SLOT, i);
    for (int32_t k = 0; k < i; ++k)   // at most 64 entries
      if (new_slot[k] == new_slot[i]) return fail(SCALE_DUP_SLOT, i);
  }
  if (P > 0 && !pair_template) return fail(SCALE_NO_PAIR_TMPL, -1);
  for (int64_t p = 0; p < P; ++p)
    if (pair_template[p] < 0 || pair_template[p] >= n_templates) return fail(SCALE_BAD_PAIR_TMPL, p);
  if (pair_max)
    for (int64_t p = 0; p < P; ++p)
      if (pair_max[p] < 0 || pair_max[p] > n_new) return fail(SCALE_BAD_PAIR_MAX, p);
  f.kmax.resize((size_t)P);
  for (int64_t i = 0; i < P; ++i) f.kmax[(size_t)i] = pair_max ? pair_max[f.fit.pairs[(size_t)i]] : n_new;
  // ---- the units again, by weight
  const size_t A = f.fit.active.size();
  f.fit.units.clear();
  for (size_t a = 0; a < A; ++a) {
    scale_cut_units((int32_t)a, f.fit.pair_start[a], f.fit.pair_start[a + 1],
                    [&](int32_t i) { return (int64_t)f.kmax[(size_t)i] + 1; }, f.fit.units);
    f.fit.unit_start[a + 1] = (int32_t)f.fit.units.size();
  }
  plan = std::move(f);
  if (bad_index) *bad_index = -1;
  return SCALE_OK;
}

}  // namespace pe

#endif  // PE_SCALE_PLAN_H_
