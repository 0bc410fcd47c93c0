// libplacement: first-fit placement of a batch over candidate domains (pe_place_first_fit_domains).  The host
// validates the batch, the hierarchy and the pair list and builds the plan (pe_first_fit_plan.h); the groups, the
// jobs, the domains' queues and the plan's words cross in one pinned block and one copy; pe_place.hip's member
// kernels gather every active domain's nodes into a compact segment, which stays the domain's working residuals;
// then ROUNDS work the queues off (launch_first_fit_round), several rounds queued per read-back of the count of
// unsettled jobs, until that count is 0; one last kernel writes the segments back
// to the live residuals.  The pod slots, statuses and pairs come back in one copy, and the host mirror and the
// stats follow from that answer.  Own buffers (pe_ctx.h ff_*): nothing of the call is kept.
#include "pe_ctx.h"
#include "pe_first_fit_plan.h"

// Rounds queued per read-back of the unsettled count: FF_ROUNDS_FIRST before the first read-back, twice as many
// before each later one, up to FF_ROUNDS_MAX (DESIGN.md section 19 has the measurement).  A batch of few rounds
// pays for few launches past its last round, a batch of thousands for one read-back in FF_ROUNDS_MAX rounds.  A
// round launched after the batch has settled finds every queue exhausted or skips settled entries: no attempt,
// no output.
#ifndef FF_ROUNDS_FIRST
#define FF_ROUNDS_FIRST 2
#endif
#ifndef FF_ROUNDS_MAX
#define FF_ROUNDS_MAX 64
#endif
static_assert(FF_ROUNDS_FIRST >= 1 && FF_ROUNDS_MAX >= FF_ROUNDS_FIRST, "FF_ROUNDS_FIRST, FF_ROUNDS_MAX");
static_assert(sizeof(pe::FirstFitCand) == sizeof(pe::FirstFitEntry), "the plan's queue entry is the device's");

namespace {

[[noreturn]] void raise_plan(pe::FitPlanError e, pe::TreePlanError te, int64_t bad) {
  switch (e) {
    case pe::FIT_BAD_LEVEL: raise(PE_EINVAL, "level outside [0, n_levels)");
    case pe::FIT_BAD_COUNT: raise(PE_EINVAL, "n_pairs outside [0, 2^31 - 1)");
    case pe::FIT_NO_PAIRS: raise(PE_EINVAL, "pair_job or pair_domain is NULL");
    case pe::FIT_BAD_JOB: raise(PE_EINVAL, "pair_job: value outside [0, n_jobs) at index " + std::to_string(bad));
    case pe::FIT_BAD_DOMAIN:
      raise(PE_EINVAL, "pair_domain: value outside [0, level_size[level]) at index " + std::to_string(bad));
    default: raise_tree(te, bad);
  }
}

}  // namespace

extern "C" {

int pe_place_first_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                               const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                               int64_t n_pairs, const int32_t* pair_job, const int32_t* pair_domain, int32_t level,
                               int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                               int32_t* out_pod_node, int32_t* out_job_status, int32_t* out_job_pair) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (ctx->world > 1)
      raise(PE_EINVAL, "pe_place_first_fit_domains on a sharded context: a domain may span shards");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::FirstFitPlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::FitPlanError err = pe::first_fit_plan_build(plan, n_jobs, job_group_off, priority, group_count, n_pairs,
                                                          pair_job, pair_domain, level, n_levels, level_size, parent, &te, &bad);
    if (err != pe::FIT_OK) raise_plan(err, te, bad);
    if (n_jobs == 0) return PE_OK;

    const int64_t J = n_jobs, NP = n_pairs, A = plan.n_active(), P = plan.pods();
    if (NP == 0) {   // no candidate anywhere: every job unschedulable, and nothing runs
      if (P > 0) std::fill(out_pod_node, out_pod_node + P, -1);
      std::fill(out_job_status, out_job_status + J, (int32_t)PE_JOB_UNSCHEDULABLE);
      if (out_job_pair) std::fill(out_job_pair, out_job_pair + J, -1);
      ctx->stats.jobs_failed += J;
      CapEvents(ctx).report_as("A=0 rounds=0");
      return PE_OK;
    }
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    int64_t with_cand = 0;   // the jobs the rounds have to settle
    for (int64_t j = 0; j < J; ++j) with_cand += plan.cand_start[(size_t)j + 1] > plan.cand_start[(size_t)j];
    // ---- one pinned block in: the groups, the jobs by index, the queues, then the plan's words
    const size_t jobs_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t queue_at = jobs_at + (size_t)J * sizeof(pe::PlaceJob);
    const size_t words_at = queue_at + (size_t)NP * sizeof(pe::FirstFitEntry);
    const size_t in_bytes = words_at + (size_t)(L0 + ND + A + 1) * sizeof(int32_t);
    hipchk(ctx->ff_hin.ensure(in_bytes), "alloc pinned first-fit inputs");
    hipchk(ctx->ff_in.ensure(in_bytes), "alloc first-fit inputs");
    pe::PlaceGroup* const h_groups = (pe::PlaceGroup*)ctx->ff_hin.p;
    for (int64_t g = 0; g < G; ++g) {
      pe::PlaceGroup& r = h_groups[g];
      std::memset(&r, 0, sizeof(r));
      for (int d = 0; d < pe::D; ++d) r.q[d] = group_req[g * pe::D + d];
      r.need = group_need ? group_need[g] : 0u;
      r.count = group_count[g];
      r.pod0 = plan.pod_off[(size_t)g];
    }
    pe::PlaceJob* const h_jobs = (pe::PlaceJob*)(ctx->ff_hin.p + jobs_at);
    for (int64_t j = 0; j < J; ++j) h_jobs[j] = pe::PlaceJob{(int32_t)j, job_group_off[j], job_group_off[j + 1], 0};
    std::memcpy(ctx->ff_hin.p + queue_at, plan.queue.data(), (size_t)NP * sizeof(pe::FirstFitEntry));
    int32_t* const h_words = (int32_t*)(ctx->ff_hin.p + words_at);
    std::memcpy(h_words, plan.leaf_dom.data(), (size_t)L0 * sizeof(int32_t));
    std::memcpy(h_words + L0, plan.act_of.data(), (size_t)ND * sizeof(int32_t));
    std::memcpy(h_words + L0 + ND, plan.q_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->ff_in.p, ctx->ff_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream),
           "H2D first-fit inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->ff_in.p;
    const pe::PlaceJob* const d_jobs = (const pe::PlaceJob*)(ctx->ff_in.p + jobs_at);
    const pe::FirstFitEntry* const d_queue = (const pe::FirstFitEntry*)(ctx->ff_in.p + queue_at);
    const int32_t* const d_words = (const int32_t*)(ctx->ff_in.p + words_at);
    const int32_t* const d_q_start = d_words + L0 + ND;
    // ---- the call's device buffers; the answers: pods [P], pairs [J], statuses [J]
    const int64_t st = std::max<int64_t>(ctx->stride, 1);
    hipchk(ctx->ff_out.ensure((size_t)(P + 2 * J)), "alloc first-fit outputs");
    hipchk(ctx->ff_hout.ensure((size_t)(P + 2 * J)), "alloc pinned first-fit outputs");
    hipchk(ctx->ff_log.ensure((size_t)(3 * P)), "alloc first-fit logs");
    hipchk(ctx->ff_dom.ensure((size_t)(3 * A + 1)), "alloc domain lists");
    hipchk(ctx->ff_seg.ensure((size_t)(pe::D * st)), "alloc domain segments");
    hipchk(ctx->ff_segw.ensure((size_t)(2 * st)), "alloc domain segments");
    hipchk(ctx->ff_state.ensure((size_t)(J + 1 + (A + 1) / 2)), "alloc first-fit state");
    hipchk(ctx->ff_hopen.ensure(1), "alloc pinned unsettled count");
    pe::PlaceSegs segs{};
    segs.cnt = ctx->ff_dom.p;
    segs.seg_off = ctx->ff_dom.p + A;
    segs.cursor = ctx->ff_dom.p + 2 * A + 1;
    segs.gid = ctx->ff_segw.p;
    segs.lab = ctx->ff_segw.p + st;
    segs.res = ctx->ff_seg.p;
    segs.seg_stride = st;
    pe::FirstFitState state{ctx->ff_state.p, (int32_t*)(ctx->ff_state.p + J + 1), (uint32_t*)(ctx->ff_state.p + J)};
    int32_t* const d_pods = ctx->ff_out.p;
    int32_t* const d_pair = ctx->ff_out.p + P;
    int32_t* const d_status = ctx->ff_out.p + P + J;
    hipchk(hipMemsetAsync(segs.cnt, 0, (size_t)A * sizeof(int32_t), ctx->stream), "zero domain counts");
    hipchk(hipMemsetAsync(state.word, 0, (size_t)(J + 1) * sizeof(uint64_t), ctx->stream), "zero first-fit state");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)state.open, (int)with_cand, 1, ctx->stream), "set unsettled count");
    hipchk(hipMemcpyAsync(state.cursor, d_q_start, (size_t)A * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream),
           "set queue cursors");
    hipchk(hipMemsetAsync(d_pods, 0xFF, (size_t)(P + J) * sizeof(int32_t), ctx->stream), "clear pods and pairs");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)PE_JOB_UNSCHEDULABLE, (size_t)J, ctx->stream),
           "preset statuses");
    CapEvents ev(ctx);
    ev.begin();
    hipchk(pe::launch_place_members(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                    (uint64_t)ctx->begin, d_words, (int)L0, d_words + L0, (int)A, segs),
           "launch place_members");
    // which of the round kernel's two instances have a segment to work on: every segment is small when the shard
    // is; otherwise the bounds come back once, and an instance without segments is never launched
    int kinds = pe::FF_SMALL;
    if (ctx->Ns > pe::PL_LDS_NODES) {
      hipchk(ctx->ff_hoff.ensure((size_t)(A + 1)), "alloc pinned segment bounds");
      hipchk(hipMemcpyAsync(ctx->ff_hoff.p, segs.seg_off, (size_t)(A + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H segment bounds");
      hipchk(hipStreamSynchronize(ctx->stream), "sync segment bounds");
      kinds = 0;
      for (int64_t a = 0; a < A; ++a)
        kinds |= ctx->ff_hoff.p[a + 1] - ctx->ff_hoff.p[a] > pe::PL_LDS_NODES ? pe::FF_LARGE : pe::FF_SMALL;
    }
    // ---- the rounds: at most n_pairs + 1 (every round attempts the lowest-ranked unsettled job at least)
    const int64_t max_rounds = NP + 1;
    int64_t rounds = 0, per_read = FF_ROUNDS_FIRST;
    uint32_t open = (uint32_t)with_cand;
    while (open > 0) {
      if (rounds >= max_rounds)
        raise(PE_EHIP, "first_fit_round_kernel: " + std::to_string(open) + " jobs unsettled after n_pairs + 1 rounds");
      const int64_t upto = std::min<int64_t>(rounds + per_read, max_rounds);
      per_read = std::min<int64_t>(2 * per_read, FF_ROUNDS_MAX);
      for (; rounds < upto; ++rounds)
        hipchk(pe::launch_first_fit_round(ctx->stream, d_groups, d_jobs, d_q_start, d_queue, (int)A, segs, kinds,
                                          (uint32_t)(rounds + 1), state, d_pods, d_status, d_pair, ctx->ff_log.p),
               "launch first_fit_round");
      hipchk(hipMemcpyAsync(ctx->ff_hopen.p, state.open, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
             "D2H unsettled count");
      hipchk(hipStreamSynchronize(ctx->stream), "sync first-fit rounds");
      open = ctx->ff_hopen.p[0];
    }
    hipchk(pe::launch_first_fit_finish(ctx->stream, segs, (int)A, ctx->Ns, ctx->res.p, ctx->stride, (uint64_t)ctx->begin),
           "launch first_fit_finish");
    ev.end();
    hipchk(hipMemcpyAsync(ctx->ff_hout.p, ctx->ff_out.p, (size_t)(P + 2 * J) * sizeof(int32_t), hipMemcpyDeviceToHost,
                          ctx->stream),
           "D2H first-fit answers");
    hipchk(hipStreamSynchronize(ctx->stream), "sync place_first_fit_domains");
    const int32_t* const pods = ctx->ff_hout.p;
    const int32_t* const pair = ctx->ff_hout.p + P;
    const int32_t* const status = ctx->ff_hout.p + P + J;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
    if (out_job_pair) std::memcpy(out_job_pair, pair, (size_t)J * sizeof(int32_t));
    // ---- the mirror follows the answer: the request off every placed pod's node, a run of one node at a time
    int64_t placed_pods = 0, placed = 0;
    for (int64_t j = 0; j < J; ++j) {
      if (status[j] != PE_JOB_PLACED) continue;
      ++placed;
      for (int64_t g = job_group_off[j]; g < job_group_off[j + 1]; ++g) {
        const int64_t p0 = plan.pod_off[(size_t)g], p1 = plan.pod_off[(size_t)g + 1];
        const int64_t* q = group_req + g * pe::D;
        placed_pods += p1 - p0;
        for (int64_t p = p0; p < p1;) {
          const int32_t node = pods[p];
          int64_t e = p + 1;
          while (e < p1 && pods[e] == node) ++e;
          if (node < 0 || node >= ctx->n_total) raise(PE_EHIP, "first_fit_round_kernel: a placed pod without a node");
          pe::NodeState& ns = ctx->m_nodes[(size_t)node];
          for (int d = 0; d < pe::D; ++d) ns.res[d] -= (e - p) * q[d];
          p = e;
        }
      }
    }
    ctx->stats.pods_placed += placed_pods;
    ctx->stats.jobs_placed += placed;
    ctx->stats.jobs_failed += J - placed;
    ev.report_as("A=" + std::to_string(A) + " rounds=" + std::to_string(rounds));
    return PE_OK;
  });
}

}  // extern "C"
