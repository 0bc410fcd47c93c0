// libplacement: gang placement inside a chosen topology domain (pe_place_greedy_domains, and
// pe_place_min_member_domains at the end of the file).  The host validates
// the batch and the hierarchy and builds the plan (pe_place_plan.h); the plan, the groups and the job records
// cross in one pinned block and one copy; the kernels of pe_place.hip gather every active domain's nodes into
// a compact segment and place each domain's jobs on it, one workgroup per domain; the pod slots and the job
// statuses come back in one copy, and the host mirror and the stats follow from that answer.  Own buffers
// (pe_ctx.h pl_*): nothing of the hierarchy or the batch is kept between calls.
#include "pe_ctx.h"
#include "pe_place_min_plan.h"
#include "pe_place_plan.h"

static_assert(pe::DM_MAX_DOMAINS == PE_MAX_DOMAINS, "PE_MAX_DOMAINS");

namespace pe_engine {

int64_t check_gang_groups(int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                          const int64_t* group_req) {
  if (n_jobs > (int64_t)INT32_MAX) raise(PE_EINVAL, "n_jobs above 2^31 - 1");
  need_ptr(job_group_off, "job_group_off");
  check_offsets(job_group_off, n_jobs, -1, "job_group_off");
  const int64_t G = job_group_off[n_jobs];
  if (G > 0) {
    need_ptr(group_count, "group_count");
    need_ptr(group_req, "group_req");
    check_req(group_req, G, "group_req");
    const int64_t i = first_bad(G, [group_count](int64_t g) { return group_count[g] < 0; });
    if (i < G) raise(PE_EINVAL, "group_count: negative value at index " + std::to_string(i));
  }
  return G;
}

void raise_tree(int tree_error, int64_t bad) {
  switch (tree_error) {
    case pe::TREE_BAD_LEVELS: raise(PE_EINVAL, "n_levels outside [1, PE_MAX_LEVELS]");
    case pe::TREE_NO_SIZES: raise(PE_EINVAL, "level_size is NULL");
    case pe::TREE_BAD_SIZE:
      raise(PE_EINVAL, "level_size: value outside [1, PE_MAX_DOMAINS] at index " + std::to_string(bad));
    case pe::TREE_NO_PARENT: raise(PE_EINVAL, "parent is NULL with n_levels > 1");
    default: raise(PE_EINVAL, "parent: value outside [-1, size of the level above) at index " + std::to_string(bad));
  }
}

// What pe_place_greedy checks of a batch (n_jobs > 0), with the first offending index; returns G.
int64_t check_place_batch(int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                          const int32_t* group_count, const int64_t* group_req, const int32_t* out_pod_node,
                          const int32_t* out_job_status) {
  if (n_jobs > (int64_t)INT32_MAX) raise(PE_EINVAL, "n_jobs above 2^31 - 1");
  need_ptr(job_group_off, "job_group_off");
  need_ptr(priority, "priority");
  need_ptr(out_job_status, "out_job_status");
  const int64_t G = check_gang_groups(n_jobs, job_group_off, group_count, group_req);
  const bool pods = first_bad(G, [group_count](int64_t g) { return group_count[g] > 0; }) < G;
  if (pods) need_ptr(out_pod_node, "out_pod_node");
  return G;
}

}  // namespace pe_engine

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

}  // namespace

extern "C" {

int pe_place_greedy_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                            const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                            const int32_t* job_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                            const int32_t* parent, int32_t* out_pod_node, int32_t* out_job_status) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (ctx->world > 1)
      raise(PE_EINVAL, "pe_place_greedy_domains on a sharded context: a domain may span shards");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::PlacePlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::PlacePlanError pe_err = pe::place_plan_build(plan, n_jobs, job_group_off, priority, group_count, job_domain,
                                                           level, n_levels, level_size, parent, &te, &bad);
    if (pe_err != pe::PLACE_OK) raise_plan(pe_err, te, bad);
    if (n_jobs == 0) return PE_OK;

    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods();
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, the jobs in plan order, then the plan's words
    const size_t jobs_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t words_at = jobs_at + (size_t)J * sizeof(pe::PlaceJob);
    const size_t n_words = (size_t)(L0 + ND + A + 1);
    const size_t in_bytes = words_at + n_words * sizeof(int32_t);
    hipchk(ctx->pl_hin.ensure(in_bytes), "alloc pinned placement inputs");
    hipchk(ctx->pl_in.ensure(in_bytes), "alloc placement inputs");
    pe::PlaceGroup* const h_groups = (pe::PlaceGroup*)ctx->pl_hin.p;
    for (int64_t g = 0; g < G; ++g) {
      pe::PlaceGroup& r = h_groups[g];
      std::memset(&r, 0, sizeof(r));
      for (int d = 0; d < pe::D; ++d) r.q[d] = group_req[g * pe::D + d];
      r.need = group_need ? group_need[g] : 0u;
      r.count = group_count[g];
      r.pod0 = plan.pod_off[(size_t)g];
    }
    pe::PlaceJob* const h_jobs = (pe::PlaceJob*)(ctx->pl_hin.p + jobs_at);
    for (int64_t i = 0; i < J; ++i) {
      const int32_t j = plan.jobs[(size_t)i];
      h_jobs[i] = pe::PlaceJob{j, job_group_off[j], job_group_off[j + 1], 0};
    }
    int32_t* const h_words = (int32_t*)(ctx->pl_hin.p + words_at);
    std::memcpy(h_words, plan.leaf_dom.data(), (size_t)L0 * sizeof(int32_t));
    std::memcpy(h_words + L0, plan.act_of.data(), (size_t)ND * sizeof(int32_t));
    std::memcpy(h_words + L0 + ND, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->pl_in.p, ctx->pl_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream),
           "H2D placement inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->pl_in.p;
    const pe::PlaceJob* const d_jobs = (const pe::PlaceJob*)(ctx->pl_in.p + jobs_at);
    const int32_t* const d_words = (const int32_t*)(ctx->pl_in.p + words_at);
    // ---- the call's device buffers
    const int64_t st = std::max<int64_t>(ctx->stride, 1);
    hipchk(ctx->pl_out.ensure((size_t)(P + J)), "alloc placement outputs");
    hipchk(ctx->pl_hout.ensure((size_t)(P + J)), "alloc pinned placement outputs");
    hipchk(ctx->pl_log.ensure((size_t)(3 * P)), "alloc placement logs");
    hipchk(ctx->pl_dom.ensure((size_t)(3 * A + 1)), "alloc domain lists");
    hipchk(ctx->pl_seg.ensure((size_t)(pe::D * st)), "alloc domain segments");
    hipchk(ctx->pl_segw.ensure((size_t)(2 * st)), "alloc domain segments");
    pe::PlaceSegs segs{};
    segs.cnt = ctx->pl_dom.p;
    segs.seg_off = ctx->pl_dom.p + A;
    segs.cursor = ctx->pl_dom.p + 2 * A + 1;
    segs.gid = ctx->pl_segw.p;
    segs.lab = ctx->pl_segw.p + st;
    segs.res = ctx->pl_seg.p;
    segs.seg_stride = st;
    hipchk(hipMemsetAsync(segs.cnt, 0, (size_t)A * sizeof(int32_t), ctx->stream), "zero domain counts");
    CapEvents ev(ctx);
    ev.begin();
    hipchk(pe::launch_place_members(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                    (uint64_t)ctx->begin, d_words, (int)L0, d_words + L0, (int)A, segs),
           "launch place_members");
    hipchk(pe::launch_place_domains(ctx->stream, d_groups, d_jobs, d_words + L0 + ND, (int)A, segs, ctx->res.p,
                                    ctx->stride, (uint64_t)ctx->begin, ctx->pl_out.p, ctx->pl_out.p + P, ctx->pl_log.p),
           "launch place_domains");
    ev.end();
    hipchk(hipMemcpyAsync(ctx->pl_hout.p, ctx->pl_out.p, (size_t)(P + J) * sizeof(int32_t), hipMemcpyDeviceToHost,
                          ctx->stream),
           "D2H placements");
    hipchk(hipStreamSynchronize(ctx->stream), "sync place_greedy_domains");
    const int32_t* const pods = ctx->pl_hout.p;
    const int32_t* const status = ctx->pl_hout.p + P;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
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
          if (node < 0 || node >= ctx->n_total) raise(PE_EHIP, "place_domains_kernel: a placed pod without a node");
          pe::NodeState& ns = ctx->m_nodes[(size_t)node];
          for (int d = 0; d < pe::D; ++d) ns.res[d] -= (e - p) * q[d];
          p = e;
        }
      }
    }
    ctx->stats.pods_placed += placed_pods;
    ctx->stats.jobs_placed += placed;
    ctx->stats.jobs_failed += J - placed;
    ev.report_as("A=" + std::to_string(A));
    return PE_OK;
  });
}

// MinMember first, the rest as fits: pe_place_greedy_domains' path with the plan of pe_place_min_plan.h, every group's
// optional share beside its record and one more block of the answer (the groups' placed pods).  The pl_*
// buffers serve both calls.
int pe_place_min_member_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                                const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                                const int32_t* min_member, const int32_t* job_domain, int32_t level, int32_t n_levels,
                                const int32_t* level_size, const int32_t* parent, int32_t* out_pod_node,
                                int32_t* out_job_status, int32_t* out_group_pods, int64_t* out_job_pods) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (ctx->world > 1)
      raise(PE_EINVAL, "pe_place_min_member_domains on a sharded context: a domain may span shards");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::PlaceMinPlan mp;
    pe::PlacePlanError be = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::PlaceMinError me =
        pe::place_min_plan_build(mp, n_jobs, job_group_off, priority, group_count, group_need, min_member, job_domain,
                                 level, n_levels, level_size, parent, &be, &te, &bad);
    if (me == pe::PLACE_MIN_BASE) raise_plan(be, te, bad);
    if (me == pe::PLACE_MIN_BELOW) raise(PE_EINVAL, "min_member: value below -1 at index " + std::to_string(bad));
    if (me == pe::PLACE_MIN_ABOVE)
      raise(PE_EINVAL, "min_member: value above the job's pod total at index " + std::to_string(bad));
    if (n_jobs == 0) return PE_OK;

    const pe::PlacePlan& plan = mp.base;
    const int64_t J = n_jobs, A = plan.n_active(), P = plan.pods(), PM = mp.mand_pods;
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the mandatory records, the optional shares, the jobs in plan order, the plan's words
    const size_t opt_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t jobs_at = opt_at + (size_t)G * sizeof(pe::PlaceMinOpt);
    const size_t words_at = jobs_at + (size_t)J * sizeof(pe::PlaceMinJob);
    const size_t n_words = (size_t)(L0 + ND + A + 1);
    const size_t in_bytes = words_at + n_words * sizeof(int32_t);
    hipchk(ctx->pl_hin.ensure(in_bytes), "alloc pinned placement inputs");
    hipchk(ctx->pl_in.ensure(in_bytes), "alloc placement inputs");
    pe::PlaceGroup* const h_groups = (pe::PlaceGroup*)ctx->pl_hin.p;
    pe::PlaceMinOpt* const h_opt = (pe::PlaceMinOpt*)(ctx->pl_hin.p + opt_at);
    for (int64_t g = 0; g < G; ++g) {
      pe::PlaceGroup& m = h_groups[g];
      std::memset(&m, 0, sizeof(m));
      for (int d = 0; d < pe::D; ++d) m.q[d] = group_req[g * pe::D + d];
      m.need = group_need ? group_need[g] : 0u;
      m.count = mp.mand[(size_t)g];
      m.pod0 = mp.mand_pod0[(size_t)g];
      h_opt[g] = pe::PlaceMinOpt{mp.opt_pod0[(size_t)g], mp.opt[(size_t)g], 0};
    }
    pe::PlaceMinJob* const h_jobs = (pe::PlaceMinJob*)(ctx->pl_hin.p + jobs_at);
    for (int64_t i = 0; i < J; ++i) {
      const int32_t j = plan.jobs[(size_t)i];
      h_jobs[i] = pe::PlaceMinJob{j,
                                  job_group_off[j],
                                  mp.job_gm[(size_t)j],
                                  job_group_off[j + 1],
                                  mp.job_shift[(size_t)j],
                                  mp.job_pods[(size_t)j]};
    }
    int32_t* const h_words = (int32_t*)(ctx->pl_hin.p + words_at);
    std::memcpy(h_words, plan.leaf_dom.data(), (size_t)L0 * sizeof(int32_t));
    std::memcpy(h_words + L0, plan.act_of.data(), (size_t)ND * sizeof(int32_t));
    std::memcpy(h_words + L0 + ND, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->pl_in.p, ctx->pl_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream),
           "H2D placement inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->pl_in.p;
    const pe::PlaceMinOpt* const d_opt = (const pe::PlaceMinOpt*)(ctx->pl_in.p + opt_at);
    const pe::PlaceMinJob* const d_jobs = (const pe::PlaceMinJob*)(ctx->pl_in.p + jobs_at);
    const int32_t* const d_words = (const int32_t*)(ctx->pl_in.p + words_at);
    // ---- the call's device buffers: one block out -- pods [P], statuses [J], the groups' placed pods [G]
    const int64_t st = std::max<int64_t>(ctx->stride, 1);
    const int64_t n_out = P + J + G;
    hipchk(ctx->pl_out.ensure((size_t)n_out), "alloc placement outputs");
    hipchk(ctx->pl_hout.ensure((size_t)n_out), "alloc pinned placement outputs");
    hipchk(ctx->pl_log.ensure((size_t)(3 * PM)), "alloc placement logs");
    hipchk(ctx->pl_dom.ensure((size_t)(3 * A + 1)), "alloc domain lists");
    hipchk(ctx->pl_seg.ensure((size_t)(pe::D * st)), "alloc domain segments");
    hipchk(ctx->pl_segw.ensure((size_t)(2 * st)), "alloc domain segments");
    pe::PlaceSegs segs{};
    segs.cnt = ctx->pl_dom.p;
    segs.seg_off = ctx->pl_dom.p + A;
    segs.cursor = ctx->pl_dom.p + 2 * A + 1;
    segs.gid = ctx->pl_segw.p;
    segs.lab = ctx->pl_segw.p + st;
    segs.res = ctx->pl_seg.p;
    segs.seg_stride = st;
    hipchk(hipMemsetAsync(segs.cnt, 0, (size_t)A * sizeof(int32_t), ctx->stream), "zero domain counts");
    if (G > 0)   // a failed job's groups hold no pod: the kernel leaves them as they are
      hipchk(hipMemsetAsync(ctx->pl_out.p + P + J, 0, (size_t)G * sizeof(int32_t), ctx->stream), "zero group pods");
    CapEvents ev(ctx);
    ev.begin();
    hipchk(pe::launch_place_members(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                    (uint64_t)ctx->begin, d_words, (int)L0, d_words + L0, (int)A, segs),
           "launch place_members");
    hipchk(pe::launch_place_min_domains(ctx->stream, d_groups, d_opt, d_jobs, d_words + L0 + ND, (int)A, segs,
                                        ctx->res.p, ctx->stride, (uint64_t)ctx->begin, ctx->pl_out.p, ctx->pl_out.p + P,
                                        ctx->pl_out.p + P + J, ctx->pl_log.p),
           "launch place_min_domains");
    ev.end();
    hipchk(hipMemcpyAsync(ctx->pl_hout.p, ctx->pl_out.p, (size_t)n_out * sizeof(int32_t), hipMemcpyDeviceToHost,
                          ctx->stream),
           "D2H placements");
    hipchk(hipStreamSynchronize(ctx->stream), "sync place_min_member_domains");
    const int32_t* const pods = ctx->pl_hout.p;
    const int32_t* const status = ctx->pl_hout.p + P;
    const int32_t* const gpods = ctx->pl_hout.p + P + J;
    if (P > 0) std::memcpy(out_pod_node, pods, (size_t)P * sizeof(int32_t));
    std::memcpy(out_job_status, status, (size_t)J * sizeof(int32_t));
    if (out_group_pods && G > 0) std::memcpy(out_group_pods, gpods, (size_t)G * sizeof(int32_t));
    // ---- the mirror follows the answer: the request off the node of every pod that holds one -- the first
    //      gpods[g] slots of group g -- a run of one node at a time
    int64_t placed_pods = 0, placed = 0;
    for (int64_t j = 0; j < J; ++j) {
      int64_t job_pods = 0;
      if (status[j] == PE_JOB_PLACED) {
        ++placed;
        for (int64_t g = job_group_off[j]; g < job_group_off[j + 1]; ++g) {
          const int64_t p0 = plan.pod_off[(size_t)g], p1 = p0 + gpods[g];
          if (gpods[g] < 0 || p1 > plan.pod_off[(size_t)g + 1])
            raise(PE_EHIP, "place_min_domains_kernel: a group's placed pods outside its count");
          const int64_t* q = group_req + g * pe::D;
          job_pods += p1 - p0;
          for (int64_t p = p0; p < p1;) {
            const int32_t node = pods[p];
            int64_t e = p + 1;
            while (e < p1 && pods[e] == node) ++e;
            if (node < 0 || node >= ctx->n_total)
              raise(PE_EHIP, "place_min_domains_kernel: a placed pod without a node");
            pe::NodeState& ns = ctx->m_nodes[(size_t)node];
            for (int d = 0; d < pe::D; ++d) ns.res[d] -= (e - p) * q[d];
            p = e;
          }
        }
      }
      if (out_job_pods) out_job_pods[j] = job_pods;
      placed_pods += job_pods;
    }
    ctx->stats.pods_placed += placed_pods;
    ctx->stats.jobs_placed += placed;
    ctx->stats.jobs_failed += J - placed;
    ev.report_as("A=" + std::to_string(A));
    return PE_OK;
  });
}

}  // extern "C"
