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
    // ---- one pinned block in: the groups, the jobs by index, the queues, then the plan's words with q_start behind
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto jobs = in.add<pe::PlaceJob>(J);
    const auto queue = in.add<pe::FirstFitEntry>(NP);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    uint8_t* const h = block_in_host(ctx, in, "first-fit");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
    pe::PlaceJob* const h_jobs = jobs.in(h);
    for (int64_t j = 0; j < J; ++j) h_jobs[j] = pe::PlaceJob{(int32_t)j, job_group_off[j], job_group_off[j + 1], 0};
    std::memcpy(queue.in(h), plan.queue.data(), queue.bytes());
    int32_t* const h_q_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_q_start, plan.q_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    const uint8_t* const d = block_in_device(ctx, in, "first-fit");
    const int32_t* const d_words = words.in(d);
    const int32_t* const d_q_start = d_words + L0 + ND;
    // ---- the call's device buffers; the answers: pods [P], pairs [J], statuses [J]
    pe::BlockLayout ans;
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto pair = ans.add<int32_t>(J, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "first-fit", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc first-fit logs");
    hipchk(ctx->ff_state.ensure((size_t)(J + 1 + (A + 1) / 2)), "alloc first-fit state");
    hipchk(ctx->ff_hopen.ensure(1), "alloc pinned unsettled count");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::FirstFitState state{ctx->ff_state.p, (int32_t*)(ctx->ff_state.p + J + 1), (uint32_t*)(ctx->ff_state.p + J)};
    int32_t* const d_pods = pods.in(o);
    int32_t* const d_status = status.in(o);
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
        hipchk(pe::launch_first_fit_round(ctx->stream, groups.in(d), jobs.in(d), d_q_start, queue.in(d), (int)A, segs, kinds,
                                          (uint32_t)(rounds + 1), state, d_pods, d_status, pair.in(o), ctx->dm_log.p),
               "launch first_fit_round");
      hipchk(hipMemcpyAsync(ctx->ff_hopen.p, state.open, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
             "D2H unsettled count");
      hipchk(hipStreamSynchronize(ctx->stream), "sync first-fit rounds");
      open = ctx->ff_hopen.p[0];
    }
    hipchk(pe::launch_first_fit_finish(ctx->stream, segs, (int)A, ctx->Ns, ctx->res.p, ctx->stride, (uint64_t)ctx->begin),
           "launch first_fit_finish");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "first-fit", "sync place_first_fit_domains");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    block_part_to(out_job_pair, pair, a);
    mirror_follow(ctx, "first_fit_round_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods.in(a), status.in(a));
    ev.report_as("A=" + std::to_string(A) + " rounds=" + std::to_string(rounds));
    return PE_OK;
  });
}

}  // extern "C"
