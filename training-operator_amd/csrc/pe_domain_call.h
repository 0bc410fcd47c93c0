// libplacement: the host scaffold of the domain calls (pe_place_greedy_domains, pe_place_min_member_domains,
// pe_gang_fit_domains, pe_place_first_fit_domains, pe_gang_preempt_domains; pe_domain_call.cpp).  Each of them
// validates, builds its plan, packs one pinned block, gathers every active domain's nodes into segments, launches
// and copies back once; what is the same in all of them is here, on the one buffer set pe_ctx.h dm_*.  Calls on a
// context are serialised (guarded), and every call sizes and fills what it reads, so one set serves them all.
#pragma once

#include "pe_ctx.h"
#include "pe_fit_plan.h"

namespace pe_engine {

// "no inventory loaded", "<call> on a sharded context: a domain may span shards", "n_jobs < 0".
void domain_entry_checks(const pe_ctx* ctx, const char* call, int64_t n_jobs);
// A refused pair list (pe_fit_plan.h FitPlanError, `bad` its index), the hierarchy in raise_tree's words.
[[noreturn]] void raise_fit_plan(pe::FitPlanError e, pe::TreePlanError te, int64_t bad);

inline size_t r16(size_t x) { return (x + 15) & ~size_t(15); }

// G zero-filled records from the caller's arrays: need 0 where group_need is NULL, pod0 0 where pod0 is NULL.
void fill_place_groups(pe::PlaceGroup* out, int64_t G, const int64_t* group_req, const uint32_t* group_need,
                       const int32_t* count, const int64_t* pod0);
// The plan's leaf_dom [n_leaf] and act_of [n_dom] back to back, the order in which every block carries them.
int32_t* pack_domain_words(int32_t* out, const std::vector<int32_t>& leaf_dom, const std::vector<int32_t>& act_of);

// The domain lists, segments and ids/labels for A active domains at the context's stride, with cnt's zeroing
// queued; then the member gather from the device copies of leaf_dom [n_leaf] and, behind it, act_of.
pe::PlaceSegs domain_segments(pe_ctx* ctx, int64_t A);
void launch_domain_members(pe_ctx* ctx, const int32_t* d_words, int64_t n_leaf, int64_t A, const pe::PlaceSegs& segs);

// The segment bounds seg_off[A + 1] on their way to dm_hoff (queued; the caller synchronises), for a shard of more
// than PL_LDS_NODES nodes: a smaller one has no segment above that.  Returns whether the copy was queued.
bool queue_segment_bounds(pe_ctx* ctx, const pe::PlaceSegs& segs, int64_t A);
// The two launches of a judging call (fit, preempt, drain, scale-up).  A segment above PL_LDS_NODES nodes needs the
// shard to have that many: only then the bounds' read-back is queued, with an event behind it; launch_units queues the LDS
// instance over the plan's units, so that the smaller segments' units already run; then the event is waited for,
// the working copies are laid out (fit_scratch_layout), the records filled, and launch_large queues the other
// instance over them -- where there is a large segment at all.
struct LargeSegs {
  const pe::FitLarge* recs = nullptr;
  int64_t n = 0;
  int64_t* scratch = nullptr;
};
void launch_units_then_large(pe_ctx* ctx, const pe::PlaceSegs& segs, int64_t A, const pe::FitPlan& plan,
                             const std::function<void()>& launch_units,
                             const std::function<void(const LargeSegs&)>& launch_large);

// The mirror and the stats follow a placing call's answer: for every placed job the request comes off the node of
// each run of equal pod slots of its groups.  pod_off [G + 1]: the groups' slots; group_pods [G] (optional): only
// the first group_pods[g] slots of group g hold a pod; out_job_pods [J] (optional): each job's placed pods.
void mirror_follow(pe_ctx* ctx, const char* kernel, int64_t J, const int32_t* job_group_off, const int64_t* group_req,
                   const int64_t* pod_off, const int32_t* pods, const int32_t* status,
                   const int32_t* group_pods = nullptr, int64_t* out_job_pods = nullptr);

}  // namespace pe_engine
