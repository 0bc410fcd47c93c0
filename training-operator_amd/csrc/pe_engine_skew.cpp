// libplacement: gang placement under maxSkew spread (pe_place_skew_domains).  pe_place_spread_domains' host path on
// the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*): the host validates the batch, the hierarchy, the
// skews, the book of existing pods and the flags and builds the plan (pe_skew_plan.h); the groups, their skews, the
// book, the job records and the plan's words cross in one pinned block and one copy; the member kernels of
// pe_place.hip gather every active domain's nodes into a compact segment, the prep kernels of pe_place_skew.hip find
// every spread domain's first place and its two instances place each domain's jobs; the pod slots, the job statuses
// and the decision counter come back in one copy.  The host mirror and the stats follow from that answer -- unless
// the call is a dry run, which leaves the device residuals, the mirror and the stats as they were.
#include "pe_domain_call.h"
#include "pe_skew_plan.h"

extern "C" {

int pe_place_skew_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                          const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                          const int32_t* group_max_skew, int32_t spread_level, const int32_t* group_base_off,
                          const int32_t* base_dom, const int32_t* base_count, uint32_t flags, const int32_t* job_domain,
                          int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                          int32_t* out_pod_node, int32_t* out_job_status) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_skew_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::SkewPlan kp;
    pe::PlacePlanError be = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const std::string at = " at index ";
    switch (pe::skew_plan_build(kp, n_jobs, job_group_off, priority, group_count, group_max_skew, spread_level,
                                group_base_off, base_dom, base_count, flags, job_domain, level, n_levels, level_size,
                                parent, ctx->n_total, &be, &te, &bad)) {
      case pe::SKEW_OK: break;
      case pe::SKEW_BAD_PLACE: raise_place_plan(be, te, bad);
      case pe::SKEW_BAD_LEVEL: raise(PE_EINVAL, "spread_level outside [-1, level)");
      case pe::SKEW_BAD_SKEW: raise(PE_EINVAL, "group_max_skew: value 0 or below -1" + at + std::to_string(bad));
      case pe::SKEW_BAD_OFF:
        if (bad < 0) raise(PE_EINVAL, "base_dom or base_count is NULL with entries in group_base_off");
        raise(PE_EINVAL, "group_base_off: negative or descending" + at + std::to_string(bad));
      case pe::SKEW_BAD_DOM: raise(PE_EINVAL, "base_dom: value outside its level" + at + std::to_string(bad));
      case pe::SKEW_BAD_COUNT: raise(PE_EINVAL, "base_count: negative value" + at + std::to_string(bad));
      case pe::SKEW_BAD_FLAGS: raise(PE_EINVAL, "flags: unknown bits");
    }
    if (n_jobs == 0) return PE_OK;

    const pe::PlacePlan& plan = kp.sp.base;
    const bool by_node = kp.by_node(), constrained = kp.constrained();
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods(), E = (int64_t)kp.book.size();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, their skews, the book, the jobs in plan order (16-B aligned), the plan's
    // words, leaf_sd
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto skews = in.add<int32_t>(G);
    const auto book_off = in.add<int32_t>(G + 1);
    const auto book = in.add<pe::SkewEntry>(E);
    const auto jobs = in.add<pe::PlaceJob>(J, 16);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    const auto leaf_sd = in.add<int32_t>(by_node ? 0 : L0);
    uint8_t* const h = block_in_host(ctx, in, "placement");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
    if (G > 0) std::memcpy(skews.in(h), kp.skew.data(), skews.bytes());
    std::memcpy(book_off.in(h), kp.book_off.data(), book_off.bytes());
    if (E > 0) std::memcpy(book.in(h), kp.book.data(), book.bytes());
    pe::PlaceJob* const h_jobs = jobs.in(h);
    for (int64_t i = 0; i < J; ++i) {
      const int32_t j = plan.jobs[(size_t)i];
      h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
    }
    int32_t* const h_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    if (!by_node) std::memcpy(leaf_sd.in(h), kp.sp.leaf_sd.data(), leaf_sd.bytes());
    const uint8_t* const d = block_in_device(ctx, in, "placement");
    const int32_t* const d_words = words.in(d);
    // ---- the call's device buffers: one block out -- the decision counter, pods [P], statuses [J] -- the logs and
    // the three scratch rows
    pe::BlockLayout ans;
    const auto made = ans.add<unsigned long long>(1, 8, true);
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "placement", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc placement logs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    const pe::SkewScratch sc = pe::skew_scratch_layout(segs.seg_stride, kp.n_keys);
    hipchk(ctx->dm_scratch.ensure((size_t)((sc.words + 1) / 2)), "alloc skew rows");
    uint32_t* const rows = (uint32_t*)ctx->dm_scratch.p;
    hipchk(hipMemsetAsync(made.in(o), 0, made.bytes(), ctx->stream), "zero the decision counter");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(pe::launch_skew_domains(ctx->stream, groups.in(d), jobs.in(d), d_words + L0 + ND, (int)A, segs, ctx->island.p,
                                   ctx->Ns, by_node ? nullptr : leaf_sd.in(d), skews.in(d), book_off.in(d),
                                   (const int32_t*)book.in(d), constrained, rows + sc.sub_at, rows + sc.cnt_at,
                                   (int32_t*)(rows + sc.where_at), kp.n_keys, ctx->res.p, ctx->stride,
                                   (uint64_t)ctx->begin, kp.dry_run, pods.in(o), status.in(o), ctx->dm_log.p, made.in(o)),
           "launch skew_domains");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "placement", "sync place_skew_domains", "D2H placements");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    if (!kp.dry_run)
      mirror_follow(ctx, "skew_domains_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods.in(a),
                    status.in(a));
    ev.report_as("A=" + std::to_string(A) + " decisions=" + std::to_string(*made.in(a)));
    return PE_OK;
  });
}

}  // extern "C"
