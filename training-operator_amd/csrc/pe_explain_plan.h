// The host plan of pe_fit_explain: the record a distinct (request, need, domain) crosses to the device as, the
// number of records one launch answers, the leaf -> level-domain map, the dedupe and the validation with its
// first offending index.  Plain C++, no HIP: the engine (pe_engine_explain.cpp) runs it once per call, and
// tests/cpp/test_explain_plan.cc runs it under the sanitizers against brute force.
#ifndef PE_EXPLAIN_PLAN_H_
#define PE_EXPLAIN_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pe_first_seen.h"
#include "pe_tree_plan.h"

namespace pe {

constexpr int EX_BINS = 32;          // PE_EXPLAIN_BINS: one per 5-bit signature
constexpr int EX_DIMS = 4;           // the resource dimensions (pe::D)
constexpr int32_t EX_ANY = -1;       // PE_EXPLAIN_ANY: the record counts every live node of the shard
constexpr int32_t EX_NO_DOMAIN = -2; // a node's level-domain when it has none: equals no record's domain
constexpr int64_t EX_OUT_WORDS = EX_BINS + EX_DIMS;                        // u64 per record on the device
constexpr int64_t EX_BUDGET_BYTES = int64_t(64) << 20;                     // a launch's result tables stay within this

// One distinct (request, need, domain): 64 B, read through a wave-uniform address with one scalar load.
struct alignas(64) ExplainRec {
  int64_t q[EX_DIMS];
  uint32_t need;
  int32_t dom;   // a level-`level` domain id, or EX_ANY
  uint32_t pad_[6];
};
static_assert(sizeof(ExplainRec) == 64, "ExplainRec is one 64-B line");

// Records per launch: as many as keep the launch's [chunk][EX_OUT_WORDS] u64 tables within budget_bytes, one at
// least, S at most.  The launches answer [0, chunk), [chunk, 2 chunk), ... up to S.
inline int64_t explain_chunk(int64_t S, int64_t budget_bytes) {
  const int64_t fit = budget_bytes / (EX_OUT_WORDS * (int64_t)sizeof(uint64_t));
  return std::max<int64_t>(1, std::min<int64_t>(S, fit));
}

// leaf_dom[level_size[0]]: the level-`level` domain of leaf domain k, walked up the parent map as
// domain_map_build does (parent[off_l + d], off_l = the sum of the sizes below level l); EX_NO_DOMAIN where the
// walk meets a -1.  The inputs are validated by the caller (explain_validate).
inline void explain_leaf_dom(int32_t level, const int32_t* level_size, const int32_t* parent,
                             std::vector<int32_t>& leaf_dom) {
  leaf_dom.resize((size_t)level_size[0]);
  for (int32_t k = 0; k < level_size[0]; ++k) {
    int32_t d = k;
    int64_t off = 0;
    for (int l = 0; l < level && d >= 0; ++l) {
      d = parent[off + d];
      off += level_size[l];
    }
    leaf_dom[(size_t)k] = d >= 0 ? d : EX_NO_DOMAIN;
  }
}

enum ExplainError {
  EX_OK = 0,
  EX_NO_REQ = 1,       // req NULL with n_jobs > 0
  EX_BAD_REQ = 2,      // a negative request; index = its place in req[j][4]
  EX_BAD_TREE = 3,     // the hierarchy is refused: *tree_error says how, index as tree_plan_build gives it
  EX_BAD_LEVEL = 4,    // level outside [0, n_levels)
  EX_BAD_DOMAIN = 5    // a job_domain outside [-1, level_size[level]); index = the job
};

// What pe_fit_explain refuses, in the order the caller sees it; *bad receives the first offending index, -1
// where the refusal has none.  With job_domain NULL the hierarchy arguments are not read.
inline ExplainError explain_validate(int64_t n_jobs, const int64_t* req, const int32_t* job_domain, int32_t level,
                                     int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                                     TreePlanError* tree_error, int64_t* bad) {
  *bad = -1;
  *tree_error = TREE_OK;
  if (n_jobs > 0 && !req) return EX_NO_REQ;
  for (int64_t i = 0; i < n_jobs * EX_DIMS; ++i)
    if (req[i] < 0) {
      *bad = i;
      return EX_BAD_REQ;
    }
  if (!job_domain) return EX_OK;
  TreePlan plan;
  *tree_error = tree_plan_build(plan, n_levels, level_size, parent, bad);
  if (*tree_error != TREE_OK) return EX_BAD_TREE;
  if (level < 0 || level >= n_levels) return EX_BAD_LEVEL;
  for (int64_t j = 0; j < n_jobs; ++j)
    if (job_domain[j] < EX_ANY || job_domain[j] >= level_size[level]) {
      *bad = j;
      return EX_BAD_DOMAIN;
    }
  return EX_OK;
}

// The batch's distinct (request, need, domain) records in first-seen order -> uniq, each job's record -> of.
// need NULL = 0, job_domain NULL = EX_ANY for every job.  Returns their number.
inline int64_t explain_dedupe(int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* job_domain,
                              std::vector<int32_t>& table, std::vector<int32_t>& of, std::vector<ExplainRec>& uniq) {
  uniq.clear();
  auto need_of = [need](int64_t j) { return need ? need[j] : 0u; };
  auto dom_of = [job_domain](int64_t j) { return job_domain ? job_domain[j] : EX_ANY; };
  return first_seen(
      n_jobs, table, of,
      [&](int64_t j) {
        uint64_t h = ((uint64_t)(uint32_t)dom_of(j) << 32) | need_of(j);
        for (int d = 0; d < EX_DIMS; ++d) h = first_seen_mix(h ^ (uint64_t)req[j * EX_DIMS + d]);
        return h;
      },
      [&](int64_t j, int32_t u) {
        const int64_t* q = req + j * EX_DIMS;
        const ExplainRec& r = uniq[(size_t)u];
        return r.q[0] == q[0] && r.q[1] == q[1] && r.q[2] == q[2] && r.q[3] == q[3] && r.need == need_of(j) &&
               r.dom == dom_of(j);
      },
      [&](int64_t j) {
        ExplainRec r{};
        for (int d = 0; d < EX_DIMS; ++d) r.q[d] = req[j * EX_DIMS + d];
        r.need = need_of(j);
        r.dom = dom_of(j);
        uniq.push_back(r);
      });
}

}  // namespace pe

#endif  // PE_EXPLAIN_PLAN_H_
