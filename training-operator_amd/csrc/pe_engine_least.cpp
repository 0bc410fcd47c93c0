// libplacement: least-allocated gang placement in rounds (pe_place_least_domains).  pe_place_greedy_domains' host
// path on the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*): the host validates the batch, the hierarchy
// and the flags and builds pe_place_greedy_domains' plan (pe_place_plan.h); the groups, the job records and the
// plan's words cross in one pinned block and one copy; the member kernels of pe_place.hip gather every active
// domain's nodes into a compact segment and the kernels of pe_place_least.hip place each domain's jobs on it; the
// pod slots, the job statuses and the decision counter come back in one copy.  The host mirror and the stats follow
// from that answer -- unless the call is a dry run, which leaves the device residuals, the mirror and the stats as
// they were.
#include "pe_domain_call.h"

extern "C" {

int pe_place_least_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                           const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                           uint32_t flags, const int32_t* job_domain, int32_t level, int32_t n_levels,
                           const int32_t* level_size, const int32_t* parent, int32_t* out_pod_node,
                           int32_t* out_job_status) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_least_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::PlacePlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::PlacePlanError be = pe::place_plan_build(plan, n_jobs, job_group_off, priority, group_count, job_domain,
                                                       level, n_levels, level_size, parent, &te, &bad);
    if (be != pe::PLACE_OK) raise_place_plan(be, te, bad);
    if (flags & ~PE_LEAST_DRY_RUN) raise(PE_EINVAL, "flags: unknown bits");
    if (n_jobs == 0) return PE_OK;

    const bool dry_run = (flags & PE_LEAST_DRY_RUN) != 0;
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, the jobs in plan order (16-B aligned), the plan's words
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto jobs = in.add<pe::PlaceJob>(J, 16);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    uint8_t* const h = block_in_host(ctx, in, "placement");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
    pe::PlaceJob* const h_jobs = jobs.in(h);
    for (int64_t i = 0; i < J; ++i) {
      const int32_t j = plan.jobs[(size_t)i];
      h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
    }
    int32_t* const h_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    const uint8_t* const d = block_in_device(ctx, in, "placement");
    const int32_t* const d_words = words.in(d);
    // ---- the call's device buffers: one block out -- the decision counter, pods [P], statuses [J] -- the logs and
    // the in-place instance's key lists
    pe::BlockLayout ans;
    const auto made = ans.add<unsigned long long>(1, 8, true);
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "placement", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc placement logs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    hipchk(ctx->dm_scratch.ensure((size_t)segs.seg_stride), "alloc round lists");
    hipchk(hipMemsetAsync(made.in(o), 0, made.bytes(), ctx->stream), "zero the decision counter");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(pe::launch_least_domains(ctx->stream, groups.in(d), jobs.in(d), d_words + L0 + ND, (int)A, segs,
                                    (uint64_t*)ctx->dm_scratch.p, ctx->res.p, ctx->stride, (uint64_t)ctx->begin, dry_run,
                                    pods.in(o), status.in(o), ctx->dm_log.p, made.in(o)),
           "launch least_domains");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "placement", "sync place_least_domains", "D2H placements");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    if (!dry_run)
      mirror_follow(ctx, "least_domains_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods.in(a),
                    status.in(a));
    ev.report_as("A=" + std::to_string(A) + " decisions=" + std::to_string(*made.in(a)));
    return PE_OK;
  });
}

}  // extern "C"
