// libplacement: gang placement inside a chosen topology domain (pe_place_greedy_domains), and MinMember first, the
// rest as fits (pe_place_min_member_domains): two entries over one body.  The host validates the batch and the
// hierarchy and builds the plan (pe_place_plan.h, pe_place_min_plan.h); the plan, the groups and the job records
// cross in one pinned block and one copy; the kernels of pe_place.hip gather every active domain's nodes into a
// compact segment and place each domain's jobs on it, one workgroup per domain (pe_place_min.hip for MinMember);
// the pod slots and the job statuses come back in one copy, and the host mirror and the stats follow from that
// answer.  The host path and the buffers are the domain calls' (pe_domain_call.h, pe_ctx.h dm_*): nothing of the
// hierarchy or the batch is kept between calls.
#include "pe_domain_call.h"
#include "pe_place_min_plan.h"

namespace {

[[noreturn]] void raise_plan(pe::PlacePlanError e, pe::TreePlanError te, int64_t bad) {
  switch (e) {
    case pe::PLACE_BAD_LEVEL: raise(PE_EINVAL, "level outside [0, n_levels)");
    case pe::PLACE_NO_DOMAINS: raise(PE_EINVAL, "job_domain is NULL");
    case pe::PLACE_BAD_DOMAIN:
      raise(PE_EINVAL, "job_domain: value outside [0, level_size[level]) at index " + std::to_string(bad));
    default: raise_tree(te, bad);   // the hierarchy, in pe_gang_capacity_tree's words
  }
}

// An entry's names in its errors.  min: pe_place_min_member_domains -- the plan of pe_place_min_plan.h, the groups'
// MANDATORY shares as their records with every group's optional share beside them, PlaceMinJob records, a log of
// the mandatory pods only and one more block of the answer (the groups' placed pods).  min_member, out_group_pods
// and out_job_pods are its alone.
struct Entry {
  bool min;
  const char *call, *sync, *launch, *kernel;
};
constexpr Entry kGreedy{false, "pe_place_greedy_domains", "sync place_greedy_domains", "launch place_domains",
                        "place_domains_kernel"};
constexpr Entry kMinMember{true, "pe_place_min_member_domains", "sync place_min_member_domains",
                           "launch place_min_domains", "place_min_domains_kernel"};

int place_in_domains(pe_ctx* ctx, const Entry& en, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                     const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                     const int32_t* min_member, const int32_t* job_domain, int32_t level, int32_t n_levels,
                     const int32_t* level_size, const int32_t* parent, int32_t* out_pod_node, int32_t* out_job_status,
                     int32_t* out_group_pods, int64_t* out_job_pods) {
  const bool min = en.min;
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, en.call, n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::PlaceMinPlan mp;   // !min: its base alone
    pe::PlacePlanError be = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    if (min) {
      const pe::PlaceMinError me =
          pe::place_min_plan_build(mp, n_jobs, job_group_off, priority, group_count, group_need, min_member, job_domain,
                                   level, n_levels, level_size, parent, &be, &te, &bad);
      if (me == pe::PLACE_MIN_BELOW) raise(PE_EINVAL, "min_member: value below -1 at index " + std::to_string(bad));
      if (me == pe::PLACE_MIN_ABOVE)
        raise(PE_EINVAL, "min_member: value above the job's pod total at index " + std::to_string(bad));
    } else {
      be = pe::place_plan_build(mp.base, n_jobs, job_group_off, priority, group_count, job_domain, level, n_levels,
                                level_size, parent, &te, &bad);
    }
    if (be != pe::PLACE_OK) raise_plan(be, te, bad);
    if (n_jobs == 0) return PE_OK;

    const pe::PlacePlan& plan = mp.base;
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, (min) their optional shares, the jobs in plan order, the plan's words
    const size_t opt_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t jobs_at = opt_at + (min ? (size_t)G * sizeof(pe::PlaceMinOpt) : 0);
    const size_t words_at = jobs_at + (size_t)J * (min ? sizeof(pe::PlaceMinJob) : sizeof(pe::PlaceJob));
    const size_t in_bytes = words_at + (size_t)(L0 + ND + A + 1) * sizeof(int32_t);
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned placement inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc placement inputs");
    uint8_t* const h = ctx->dm_hin.p;
    if (min) {
      fill_place_groups((pe::PlaceGroup*)h, G, group_req, group_need, mp.mand.data(), mp.mand_pod0.data());
      pe::PlaceMinOpt* const h_opt = (pe::PlaceMinOpt*)(h + opt_at);
      for (int64_t g = 0; g < G; ++g) h_opt[g] = pe::PlaceMinOpt{mp.opt_pod0[(size_t)g], mp.opt[(size_t)g], 0};
      pe::PlaceMinJob* const h_jobs = (pe::PlaceMinJob*)(h + jobs_at);
      for (int64_t i = 0; i < J; ++i) {
        const int32_t j = plan.jobs[(size_t)i];
        h_jobs[i] = pe::PlaceMinJob{j,
                                    job_group_off[j],
                                    mp.job_gm[(size_t)j],
                                    job_group_off[j + 1],
                                    mp.job_shift[(size_t)j],
                                    mp.job_pods[(size_t)j]};
      }
    } else {
      fill_place_groups((pe::PlaceGroup*)h, G, group_req, group_need, group_count, plan.pod_off.data());
      pe::PlaceJob* const h_jobs = (pe::PlaceJob*)(h + jobs_at);
      for (int64_t i = 0; i < J; ++i) {
        const int32_t j = plan.jobs[(size_t)i];
        h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
      }
    }
    int32_t* const h_start = pack_domain_words((int32_t*)(h + words_at), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->dm_in.p, h, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D placement inputs");
    const uint8_t* const d = ctx->dm_in.p;
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)d;
    const int32_t* const d_words = (const int32_t*)(d + words_at);
    // ---- the call's device buffers: one block out -- pods [P], statuses [J], (min) the groups' placed pods [G]
    const int64_t n_out = P + J + (min ? G : 0);
    hipchk(ctx->dm_out.ensure((size_t)n_out * sizeof(int32_t)), "alloc placement outputs");
    hipchk(ctx->dm_hout.ensure((size_t)n_out * sizeof(int32_t)), "alloc pinned placement outputs");
    hipchk(ctx->dm_log.ensure((size_t)(3 * (min ? mp.mand_pods : P))), "alloc placement logs");
    int32_t* const d_out = (int32_t*)ctx->dm_out.p;
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    if (min && G > 0)   // a failed job's groups hold no pod: the kernel leaves them as they are
      hipchk(hipMemsetAsync(d_out + P + J, 0, (size_t)G * sizeof(int32_t), ctx->stream), "zero group pods");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(min ? pe::launch_place_min_domains(ctx->stream, d_groups, (const pe::PlaceMinOpt*)(d + opt_at),
                                              (const pe::PlaceMinJob*)(d + jobs_at), d_words + L0 + ND, (int)A, segs,
                                              ctx->res.p, ctx->stride, (uint64_t)ctx->begin, d_out, d_out + P,
                                              d_out + P + J, ctx->dm_log.p)
               : pe::launch_place_domains(ctx->stream, d_groups, (const pe::PlaceJob*)(d + jobs_at), d_words + L0 + ND,
                                          (int)A, segs, ctx->res.p, ctx->stride, (uint64_t)ctx->begin, d_out, d_out + P,
                                          ctx->dm_log.p),
           en.launch);
    ev.end();
    hipchk(hipMemcpyAsync(ctx->dm_hout.p, d_out, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream),
           "D2H placements");
    hipchk(hipStreamSynchronize(ctx->stream), en.sync);
    const int32_t* const pods = (const int32_t*)ctx->dm_hout.p;
    const int32_t* const status = pods + P;
    const int32_t* const gpods = min ? pods + P + J : nullptr;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
    if (min && out_group_pods && G > 0) std::memcpy(out_group_pods, gpods, (size_t)G * sizeof(int32_t));
    mirror_follow(ctx, en.kernel, J, job_group_off, group_req, plan.pod_off.data(), pods, status, gpods,
                  min ? out_job_pods : nullptr);
    ev.report_as("A=" + std::to_string(A));
    return PE_OK;
  });
}

}  // namespace

extern "C" {

int pe_place_greedy_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                            const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                            const int32_t* job_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                            const int32_t* parent, int32_t* out_pod_node, int32_t* out_job_status) {
  return place_in_domains(ctx, kGreedy, n_jobs, job_group_off, priority, group_count, group_req, group_need, nullptr,
                          job_domain, level, n_levels, level_size, parent, out_pod_node, out_job_status, nullptr, nullptr);
}

int pe_place_min_member_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                                const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                                const int32_t* min_member, const int32_t* job_domain, int32_t level, int32_t n_levels,
                                const int32_t* level_size, const int32_t* parent, int32_t* out_pod_node,
                                int32_t* out_job_status, int32_t* out_group_pods, int64_t* out_job_pods) {
  return place_in_domains(ctx, kMinMember, n_jobs, job_group_off, priority, group_count, group_req, group_need, min_member,
                          job_domain, level, n_levels, level_size, parent, out_pod_node, out_job_status, out_group_pods,
                          out_job_pods);
}

}  // extern "C"
