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
    if (be != pe::PLACE_OK) raise_place_plan(be, te, bad);
    if (n_jobs == 0) return PE_OK;

    const pe::PlacePlan& plan = mp.base;
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, (min) their optional shares, the jobs in plan order, the plan's words
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto opt = in.add<pe::PlaceMinOpt>(min ? G : 0);
    const auto jobs = in.add<pe::PlaceJob>(min ? 0 : J);
    const auto mjobs = in.add<pe::PlaceMinJob>(min ? J : 0);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    uint8_t* const h = block_in_host(ctx, in, "placement");
    if (min) {
      fill_place_groups(groups.in(h), G, group_req, group_need, mp.mand.data(), mp.mand_pod0.data());
      pe::PlaceMinOpt* const h_opt = opt.in(h);
      for (int64_t g = 0; g < G; ++g) h_opt[g] = pe::PlaceMinOpt{mp.opt_pod0[(size_t)g], mp.opt[(size_t)g], 0};
      pe::PlaceMinJob* const h_jobs = mjobs.in(h);
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
      fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
      pe::PlaceJob* const h_jobs = jobs.in(h);
      for (int64_t i = 0; i < J; ++i) {
        const int32_t j = plan.jobs[(size_t)i];
        h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
      }
    }
    int32_t* const h_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    const uint8_t* const d = block_in_device(ctx, in, "placement");
    const int32_t* const d_words = words.in(d);
    // ---- the call's device buffers: one block out -- pods [P], statuses [J], (min) the groups' placed pods [G]
    pe::BlockLayout ans;
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    const auto gpods = ans.add<int32_t>(min ? G : 0, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "placement", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * (min ? mp.mand_pods : P))), "alloc placement logs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    if (min && G > 0)   // a failed job's groups hold no pod: the kernel leaves them as they are
      hipchk(hipMemsetAsync(gpods.in(o), 0, gpods.bytes(), ctx->stream), "zero group pods");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(min ? pe::launch_place_min_domains(ctx->stream, groups.in(d), opt.in(d), mjobs.in(d), d_words + L0 + ND, (int)A,
                                              segs, ctx->res.p, ctx->stride, (uint64_t)ctx->begin, pods.in(o),
                                              status.in(o), gpods.in(o), ctx->dm_log.p)
               : pe::launch_place_domains(ctx->stream, groups.in(d), jobs.in(d), d_words + L0 + ND, (int)A, segs,
                                          ctx->res.p, ctx->stride, (uint64_t)ctx->begin, pods.in(o), status.in(o),
                                          ctx->dm_log.p),
           en.launch);
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "placement", en.sync, "D2H placements");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    block_part_to(out_group_pods, gpods, a);
    mirror_follow(ctx, en.kernel, J, job_group_off, group_req, plan.pod_off.data(), pods.in(a), status.in(a),
                  min ? gpods.in(a) : nullptr, min ? out_job_pods : nullptr);
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
