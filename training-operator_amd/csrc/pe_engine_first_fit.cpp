// libplacement: first-fit placement of a batch over candidate domains (pe_place_first_fit_domains).  The host
// validates the batch, the hierarchy and the pair list and builds the plan (pe_first_fit_plan.h); the groups, the
// jobs, the domains' queues and the plan's words cross in one pinned block and one copy; pe_place.hip's member
// kernels gather every active domain's nodes into a compact segment, which stays the domain's working residuals;
// then ROUNDS work the queues off (launch_first_fit_round), several rounds queued per read-back of the count of
// unsettled jobs, until that count is 0; one last kernel writes the segments back
// to the live residuals.  The pod slots, statuses and pairs come back in one copy, and the host mirror and the
// stats follow from that answer.  The host path and the buffers are the domain calls' (pe_domain_call.h, pe_ctx.h
// dm_*, ff_state and ff_hopen): nothing of the call is kept.
#include "pe_domain_call.h"
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

extern "C" {

int pe_place_first_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                               const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                               int64_t n_pairs, const int32_t* pair_job, const int32_t* pair_domain, int32_t level,
                               int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                               int32_t* out_pod_node, int32_t* out_job_status, int32_t* out_job_pair) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_first_fit_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::FirstFitPlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::FitPlanError err = pe::first_fit_plan_build(plan, n_jobs, job_group_off, priority, group_count, n_pairs,
                                                          pair_job, pair_domain, level, n_levels, level_size, parent, &te, &bad);
    if (err != pe::FIT_OK) raise_fit_plan(err, te, bad);
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
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned first-fit inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc first-fit inputs");
    fill_place_groups((pe::PlaceGroup*)ctx->dm_hin.p, G, group_req, group_need, group_count, plan.pod_off.data());
    pe::PlaceJob* const h_jobs = (pe::PlaceJob*)(ctx->dm_hin.p + jobs_at);
    for (int64_t j = 0; j < J; ++j) h_jobs[j] = pe::PlaceJob{(int32_t)j, job_group_off[j], job_group_off[j + 1], 0};
    std::memcpy(ctx->dm_hin.p + queue_at, plan.queue.data(), (size_t)NP * sizeof(pe::FirstFitEntry));
    int32_t* const h_q_start = pack_domain_words((int32_t*)(ctx->dm_hin.p + words_at), plan.leaf_dom, plan.act_of);
    std::memcpy(h_q_start, plan.q_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->dm_in.p, ctx->dm_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream),
           "H2D first-fit inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->dm_in.p;
    const pe::PlaceJob* const d_jobs = (const pe::PlaceJob*)(ctx->dm_in.p + jobs_at);
    const pe::FirstFitEntry* const d_queue = (const pe::FirstFitEntry*)(ctx->dm_in.p + queue_at);
    const int32_t* const d_words = (const int32_t*)(ctx->dm_in.p + words_at);
    const int32_t* const d_q_start = d_words + L0 + ND;
    // ---- the call's device buffers; the answers: pods [P], pairs [J], statuses [J]
    const size_t out_bytes = (size_t)(P + 2 * J) * sizeof(int32_t);
    hipchk(ctx->dm_out.ensure(out_bytes), "alloc first-fit outputs");
    hipchk(ctx->dm_hout.ensure(out_bytes), "alloc pinned first-fit outputs");
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc first-fit logs");
    hipchk(ctx->ff_state.ensure((size_t)(J + 1 + (A + 1) / 2)), "alloc first-fit state");
    hipchk(ctx->ff_hopen.ensure(1), "alloc pinned unsettled count");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::FirstFitState state{ctx->ff_state.p, (int32_t*)(ctx->ff_state.p + J + 1), (uint32_t*)(ctx->ff_state.p + J)};
    int32_t* const d_pods = (int32_t*)ctx->dm_out.p;
    int32_t* const d_pair = d_pods + P;
    int32_t* const d_status = d_pods + P + J;
    hipchk(hipMemsetAsync(state.word, 0, (size_t)(J + 1) * sizeof(uint64_t), ctx->stream), "zero first-fit state");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)state.open, (int)with_cand, 1, ctx->stream), "set unsettled count");
    hipchk(hipMemcpyAsync(state.cursor, d_q_start, (size_t)A * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream),
           "set queue cursors");
    hipchk(hipMemsetAsync(d_pods, 0xFF, (size_t)(P + J) * sizeof(int32_t), ctx->stream), "clear pods and pairs");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)PE_JOB_UNSCHEDULABLE, (size_t)J, ctx->stream),
           "preset statuses");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    // which of the round kernel's two instances have a segment to work on: every segment is small when the shard
    // is; otherwise the bounds come back once, and an instance without segments is never launched
    int kinds = pe::FF_SMALL;
    if (queue_segment_bounds(ctx, segs, A)) {
      hipchk(hipStreamSynchronize(ctx->stream), "sync segment bounds");
      kinds = 0;
      for (int64_t a = 0; a < A; ++a)
        kinds |= ctx->dm_hoff.p[a + 1] - ctx->dm_hoff.p[a] > pe::PL_LDS_NODES ? pe::FF_LARGE : pe::FF_SMALL;
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
                                          (uint32_t)(rounds + 1), state, d_pods, d_status, d_pair, ctx->dm_log.p),
               "launch first_fit_round");
      hipchk(hipMemcpyAsync(ctx->ff_hopen.p, state.open, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
             "D2H unsettled count");
      hipchk(hipStreamSynchronize(ctx->stream), "sync first-fit rounds");
      open = ctx->ff_hopen.p[0];
    }
    hipchk(pe::launch_first_fit_finish(ctx->stream, segs, (int)A, ctx->Ns, ctx->res.p, ctx->stride, (uint64_t)ctx->begin),
           "launch first_fit_finish");
    ev.end();
    hipchk(hipMemcpyAsync(ctx->dm_hout.p, ctx->dm_out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream),
           "D2H first-fit answers");
    hipchk(hipStreamSynchronize(ctx->stream), "sync place_first_fit_domains");
    const int32_t* const pods = (const int32_t*)ctx->dm_hout.p;
    const int32_t* const pair = pods + P;
    const int32_t* const status = pods + P + J;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
    if (out_job_pair) std::memcpy(out_job_pair, pair, (size_t)J * sizeof(int32_t));
    mirror_follow(ctx, "first_fit_round_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods, status);
    ev.report_as("A=" + std::to_string(A) + " rounds=" + std::to_string(rounds));
    return PE_OK;
  });
}

}  // extern "C"
