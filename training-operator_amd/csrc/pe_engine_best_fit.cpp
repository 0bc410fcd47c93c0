// libplacement: best-fit placement of a batch over candidate domains (pe_place_best_fit_domains).  First fit's host
// path (pe_engine_first_fit.cpp) on the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*, ff_state and
// ff_hopen): the host validates the batch, the hierarchy, the pair list and the flags and builds the plan
// (pe_best_fit_plan.h); the groups, the jobs, the kept pairs, the queues and the plan's words cross in one pinned
// block and one copy; pe_place.hip's member kernels gather every active domain's nodes into a compact segment, which
// stays the domain's working residuals; then ROUNDS evaluate and decide (launch_best_fit_round), several rounds
// queued per read-back of the count of unsettled jobs, until that count is 0; first fit's last kernel writes the
// segments back to the live residuals -- unless the call is a dry run, which leaves the device residuals, the mirror
// and the stats as they were.  The pod slots, statuses, pairs and the pairs' slots come back in one copy.
#include "pe_best_fit_plan.h"
#include "pe_domain_call.h"

// Rounds queued per read-back of the unsettled count: first fit's cadence.
#ifndef BF_ROUNDS_FIRST
#define BF_ROUNDS_FIRST 2
#endif
#ifndef BF_ROUNDS_MAX
#define BF_ROUNDS_MAX 64
#endif
static_assert(BF_ROUNDS_FIRST >= 1 && BF_ROUNDS_MAX >= BF_ROUNDS_FIRST, "BF_ROUNDS_FIRST, BF_ROUNDS_MAX");
static_assert(sizeof(pe::BestFitCand) == sizeof(pe::BestFitEntry), "the plan's queue entry is the device's");
static_assert(PE_PAIR_NO_FIT == -1, "ev_slots' cell for a pair that does not fit");

extern "C" {

int pe_place_best_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                              const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                              int64_t n_pairs, const int32_t* pair_job, const int32_t* pair_domain, uint32_t flags,
                              int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                              int32_t* out_pod_node, int32_t* out_job_status, int32_t* out_job_pair,
                              int64_t* out_pair_slots) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_best_fit_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::BestFitPlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::FitPlanError err = pe::best_fit_plan_build(plan, n_jobs, job_group_off, priority, group_count, n_pairs,
                                                         pair_job, pair_domain, level, n_levels, level_size, parent, &te, &bad);
    if (err != pe::FIT_OK) raise_fit_plan(err, te, bad);
    if (flags & ~PE_BEST_DRY_RUN) raise(PE_EINVAL, "flags: unknown bits");
    if (n_jobs == 0) return PE_OK;

    const bool dry_run = (flags & PE_BEST_DRY_RUN) != 0;
    const int64_t J = n_jobs, NP = n_pairs, K = plan.n_kept(), A = plan.n_active(), P = plan.pods();
    if (NP == 0) {   // no candidate anywhere: every job unschedulable, and nothing runs
      if (P > 0) std::fill(out_pod_node, out_pod_node + P, -1);
      std::fill(out_job_status, out_job_status + J, (int32_t)PE_JOB_UNSCHEDULABLE);
      if (out_job_pair) std::fill(out_job_pair, out_job_pair + J, -1);
      if (!dry_run) ctx->stats.jobs_failed += J;
      CapEvents(ctx).report_as("A=0 rounds=0");
      return PE_OK;
    }
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    int64_t with_cand = 0;   // the jobs the rounds have to settle
    for (int64_t j = 0; j < J; ++j) with_cand += plan.kept_start[(size_t)j + 1] > plan.kept_start[(size_t)j];
    // ---- one pinned block in: the groups, the jobs by index, the queues, the kept pairs, then the plan's words with
    // q_start behind
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto jobs = in.add<pe::BestFitJob>(J, 32);
    const auto queue = in.add<pe::BestFitEntry>(K);
    const auto kept = in.add<int32_t>(K);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    uint8_t* const h = block_in_host(ctx, in, "best-fit");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
    pe::BestFitJob* const h_jobs = jobs.in(h);
    for (int64_t j = 0; j < J; ++j)
      h_jobs[j] = pe::BestFitJob{job_group_off[j], job_group_off[j + 1], plan.ref_group[(size_t)j],
                                 plan.kept_start[(size_t)j], plan.kept_start[(size_t)j + 1], {0, 0, 0}};
    std::memcpy(queue.in(h), plan.queue.data(), queue.bytes());
    std::memcpy(kept.in(h), plan.kept.data(), kept.bytes());
    int32_t* const h_q_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_q_start, plan.q_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    const uint8_t* const d = block_in_device(ctx, in, "best-fit");
    const int32_t* const d_words = words.in(d);
    const int32_t* const d_q_start = d_words + L0 + ND;
    // ---- the call's device buffers; the answers: the pairs' slots [NP], pods [P], pairs [J], statuses [J]
    pe::BlockLayout ans;
    const auto slots = ans.add<long long>(NP, 8, true);
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto pair = ans.add<int32_t>(J, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "best-fit", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc best-fit logs");
    // the rounds' state: the unsettled count, the queue cursors [A], the pairs' stamps [NP]
    hipchk(ctx->ff_state.ensure((size_t)(1 + (A + 1) / 2 + (NP + 1) / 2)), "alloc best-fit state");
    hipchk(ctx->ff_hopen.ensure(1), "alloc pinned unsettled count");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    uint32_t* const d_open = (uint32_t*)ctx->ff_state.p;
    int32_t* const d_cursor = (int32_t*)(ctx->ff_state.p + 1);
    uint32_t* const d_round = (uint32_t*)(ctx->ff_state.p + 1 + (A + 1) / 2);
    const pe::BestFitState state{d_round, slots.in(o), d_cursor, d_open};
    int32_t* const d_pods = pods.in(o);
    int32_t* const d_status = status.in(o);
    hipchk(hipMemsetAsync(d_round, 0, (size_t)NP * sizeof(uint32_t), ctx->stream), "zero best-fit stamps");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)d_open, (int)with_cand, 1, ctx->stream), "set unsettled count");
    hipchk(hipMemcpyAsync(d_cursor, d_q_start, (size_t)A * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream),
           "set queue cursors");
    hipchk(hipMemsetAsync(slots.in(o), 0xFF, slots.bytes(), ctx->stream), "preset the pairs' slots");
    hipchk(hipMemsetAsync(d_pods, 0xFF, (size_t)(P + J) * sizeof(int32_t), ctx->stream), "clear pods and pairs");
    hipchk(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)PE_JOB_UNSCHEDULABLE, (size_t)J, ctx->stream),
           "preset statuses");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    // which of the round kernel's two instances have a segment to work on, as first fit finds out; the in-place
    // instance walks its evaluations on a shadow of the segments' rows
    int kinds = pe::FF_SMALL;
    if (queue_segment_bounds(ctx, segs, A)) {
      hipchk(hipStreamSynchronize(ctx->stream), "sync segment bounds");
      kinds = 0;
      for (int64_t a = 0; a < A; ++a)
        kinds |= ctx->dm_hoff.p[a + 1] - ctx->dm_hoff.p[a] > pe::PL_LDS_NODES ? pe::FF_LARGE : pe::FF_SMALL;
    }
    if (kinds & pe::FF_LARGE) hipchk(ctx->dm_scratch.ensure((size_t)(pe::D * segs.seg_stride)), "alloc segment shadows");
    // ---- the rounds: every round evaluates a kept pair or settles a job, so at most K + J of them; one to spare
    const int64_t max_rounds = NP + J + 1;
    int64_t rounds = 0, per_read = BF_ROUNDS_FIRST;
    uint32_t open = (uint32_t)with_cand;
    while (open > 0) {
      if (rounds >= max_rounds)
        raise(PE_EHIP, "best_fit_round_kernel: " + std::to_string(open) + " jobs unsettled after n_pairs + n_jobs + 1 rounds");
      const int64_t upto = std::min<int64_t>(rounds + per_read, max_rounds);
      per_read = std::min<int64_t>(2 * per_read, BF_ROUNDS_MAX);
      for (; rounds < upto; ++rounds)
        hipchk(pe::launch_best_fit_round(ctx->stream, groups.in(d), jobs.in(d), kept.in(d), d_q_start, queue.in(d), (int)A,
                                         segs, (kinds & pe::FF_LARGE) ? ctx->dm_scratch.p : nullptr, kinds,
                                         (uint32_t)(rounds + 1), state, d_pods, d_status, pair.in(o), ctx->dm_log.p),
               "launch best_fit_round");
      hipchk(hipMemcpyAsync(ctx->ff_hopen.p, state.open, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
             "D2H unsettled count");
      hipchk(hipStreamSynchronize(ctx->stream), "sync best-fit rounds");
      open = ctx->ff_hopen.p[0];
    }
    if (!dry_run)
      hipchk(pe::launch_first_fit_finish(ctx->stream, segs, (int)A, ctx->Ns, ctx->res.p, ctx->stride, (uint64_t)ctx->begin),
             "launch first_fit_finish");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "best-fit", "sync place_best_fit_domains");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    block_part_to(out_job_pair, pair, a);
    if (out_pair_slots)
      for (int64_t p = 0; p < NP; ++p)
        out_pair_slots[p] = plan.repeat[(size_t)p] ? (int64_t)PE_PAIR_REPEAT : (int64_t)slots.in(a)[p];
    if (!dry_run)
      mirror_follow(ctx, "best_fit_round_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods.in(a), status.in(a));
    ev.report_as("A=" + std::to_string(A) + " rounds=" + std::to_string(rounds));
    return PE_OK;
  });
}

}  // extern "C"
