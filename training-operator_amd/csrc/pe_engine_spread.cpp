// libplacement: gang placement with per-domain pod caps (pe_place_spread_domains).  pe_place_greedy_domains' host
// path on the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*): the host validates the batch, the hierarchy,
// the caps and the flags and builds the plan (pe_spread_plan.h); the groups, their caps, the job records and the
// plan's words cross in one pinned block and one copy; the member kernels of pe_place.hip gather every active
// domain's nodes into a compact segment and the kernels of pe_spread.hip place each domain's jobs on it; the pod
// slots and the job statuses come back in one copy.  The host mirror and the stats follow from that answer --
// unless the call is a dry run, which leaves the device residuals, the mirror and the stats as they were.
#include "pe_domain_call.h"
#include "pe_spread_plan.h"

extern "C" {

int pe_place_spread_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                            const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                            const int32_t* group_max_per, int32_t spread_level, uint32_t flags, const int32_t* job_domain,
                            int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                            int32_t* out_pod_node, int32_t* out_job_status) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_spread_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::SpreadPlan sp;
    pe::PlacePlanError be = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    switch (pe::spread_plan_build(sp, n_jobs, job_group_off, priority, group_count, group_max_per, spread_level, flags,
                                  job_domain, level, n_levels, level_size, parent, &be, &te, &bad)) {
      case pe::SPREAD_OK: break;
      case pe::SPREAD_BAD_PLACE: raise_place_plan(be, te, bad);
      case pe::SPREAD_BAD_LEVEL: raise(PE_EINVAL, "spread_level outside [-1, level)");
      case pe::SPREAD_BAD_CAP:
        raise(PE_EINVAL, "group_max_per: value 0 or below -1 at index " + std::to_string(bad));
      case pe::SPREAD_BAD_FLAGS: raise(PE_EINVAL, "flags: unknown bits");
    }
    if (n_jobs == 0) return PE_OK;

    const pe::PlacePlan& plan = sp.base;
    const bool by_node = sp.by_node();
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, their caps, the jobs in plan order, the plan's words, leaf_sub
    const size_t caps_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t jobs_at = r16(caps_at + (size_t)G * sizeof(int32_t));
    const size_t words_at = jobs_at + (size_t)J * sizeof(pe::PlaceJob);
    const size_t sub_at = words_at + (size_t)(L0 + ND + A + 1) * sizeof(int32_t);
    const size_t in_bytes = sub_at + (by_node ? 0 : (size_t)L0 * sizeof(int32_t));
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned placement inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc placement inputs");
    uint8_t* const h = ctx->dm_hin.p;
    fill_place_groups((pe::PlaceGroup*)h, G, group_req, group_need, group_count, plan.pod_off.data());
    if (G > 0) std::memcpy(h + caps_at, sp.cap.data(), (size_t)G * sizeof(int32_t));
    pe::PlaceJob* const h_jobs = (pe::PlaceJob*)(h + jobs_at);
    for (int64_t i = 0; i < J; ++i) {
      const int32_t j = plan.jobs[(size_t)i];
      h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
    }
    int32_t* const h_start = pack_domain_words((int32_t*)(h + words_at), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    if (!by_node) std::memcpy(h + sub_at, sp.leaf_sub.data(), (size_t)L0 * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->dm_in.p, h, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D placement inputs");
    const uint8_t* const d = ctx->dm_in.p;
    const int32_t* const d_words = (const int32_t*)(d + words_at);
    // ---- the call's device buffers: one block out -- pods [P], statuses [J] -- the logs and the two scratch rows
    const int64_t n_out = P + J;
    hipchk(ctx->dm_out.ensure((size_t)n_out * sizeof(int32_t)), "alloc placement outputs");
    hipchk(ctx->dm_hout.ensure((size_t)n_out * sizeof(int32_t)), "alloc pinned placement outputs");
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc placement logs");
    int32_t* const d_out = (int32_t*)ctx->dm_out.p;
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    const pe::SpreadScratch sc = pe::spread_scratch_layout(segs.seg_stride, by_node);
    hipchk(ctx->dm_scratch.ensure((size_t)((sc.words + 1) / 2)), "alloc allowance rows");
    uint32_t* const rows = (uint32_t*)ctx->dm_scratch.p;
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(pe::launch_spread_domains(ctx->stream, (const pe::PlaceGroup*)d, (const int32_t*)(d + caps_at),
                                     (const pe::PlaceJob*)(d + jobs_at), d_words + L0 + ND, (int)A, segs, ctx->island.p,
                                     ctx->Ns, by_node ? nullptr : (const int32_t*)(d + sub_at), rows + sc.allow_at,
                                     rows + sc.sub_at, ctx->res.p, ctx->stride, (uint64_t)ctx->begin, sp.dry_run, d_out,
                                     d_out + P, ctx->dm_log.p),
           "launch spread_domains");
    ev.end();
    hipchk(hipMemcpyAsync(ctx->dm_hout.p, d_out, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream),
           "D2H placements");
    hipchk(hipStreamSynchronize(ctx->stream), "sync place_spread_domains");
    const int32_t* const pods = (const int32_t*)ctx->dm_hout.p;
    const int32_t* const status = pods + P;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
    if (!sp.dry_run)
      mirror_follow(ctx, "spread_domains_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods, status);
    ev.report_as("A=" + std::to_string(A));
    return PE_OK;
  });
}

}  // extern "C"
