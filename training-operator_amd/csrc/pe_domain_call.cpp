// libplacement: the host scaffold of the domain calls (pe_domain_call.h).
#include "pe_domain_call.h"

static_assert(pe::DM_MAX_DOMAINS == PE_MAX_DOMAINS, "PE_MAX_DOMAINS");

namespace pe_engine {

void domain_entry_checks(const pe_ctx* ctx, const char* call, int64_t n_jobs) {
  if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
  if (ctx->world > 1) raise(PE_EINVAL, std::string(call) + " on a sharded context: a domain may span shards");
  if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
}

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

void raise_fit_plan(pe::FitPlanError e, pe::TreePlanError te, int64_t bad) {
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

void fill_place_groups(pe::PlaceGroup* out, int64_t G, const int64_t* group_req, const uint32_t* group_need,
                       const int32_t* count, const int64_t* pod0) {
  for (int64_t g = 0; g < G; ++g) {
    pe::PlaceGroup& r = out[g];
    std::memset(&r, 0, sizeof(r));
    for (int d = 0; d < pe::D; ++d) r.q[d] = group_req[g * pe::D + d];
    r.need = group_need ? group_need[g] : 0u;
    r.count = count[g];
    if (pod0) r.pod0 = pod0[g];
  }
}

int32_t* pack_domain_words(int32_t* out, const std::vector<int32_t>& leaf_dom, const std::vector<int32_t>& act_of) {
  std::memcpy(out, leaf_dom.data(), leaf_dom.size() * sizeof(int32_t));
  std::memcpy(out + leaf_dom.size(), act_of.data(), act_of.size() * sizeof(int32_t));
  return out + leaf_dom.size() + act_of.size();
}

pe::PlaceSegs domain_segments(pe_ctx* ctx, int64_t A) {
  const int64_t st = std::max<int64_t>(ctx->stride, 1);
  hipchk(ctx->dm_dom.ensure((size_t)(3 * A + 1)), "alloc domain lists");
  hipchk(ctx->dm_seg.ensure((size_t)(pe::D * st)), "alloc domain segments");
  hipchk(ctx->dm_segw.ensure((size_t)(2 * st)), "alloc domain segments");
  pe::PlaceSegs segs{};
  segs.cnt = ctx->dm_dom.p;
  segs.seg_off = ctx->dm_dom.p + A;
  segs.cursor = ctx->dm_dom.p + 2 * A + 1;
  segs.gid = ctx->dm_segw.p;
  segs.lab = ctx->dm_segw.p + st;
  segs.res = ctx->dm_seg.p;
  segs.seg_stride = st;
  hipchk(hipMemsetAsync(segs.cnt, 0, (size_t)A * sizeof(int32_t), ctx->stream), "zero domain counts");
  return segs;
}

void launch_domain_members(pe_ctx* ctx, const int32_t* d_words, int64_t n_leaf, int64_t A, const pe::PlaceSegs& segs) {
  hipchk(pe::launch_place_members(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                  (uint64_t)ctx->begin, d_words, (int)n_leaf, d_words + n_leaf, (int)A, segs),
         "launch place_members");
}

bool queue_segment_bounds(pe_ctx* ctx, const pe::PlaceSegs& segs, int64_t A) {
  if (ctx->Ns <= pe::PL_LDS_NODES) return false;
  hipchk(ctx->dm_hoff.ensure((size_t)(A + 1)), "alloc pinned segment bounds");
  hipchk(hipMemcpyAsync(ctx->dm_hoff.p, segs.seg_off, (size_t)(A + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                        ctx->stream),
         "D2H segment bounds");
  return true;
}

void launch_units_then_large(pe_ctx* ctx, const pe::PlaceSegs& segs, int64_t A, const pe::FitPlan& plan,
                             const std::function<void()>& launch_units,
                             const std::function<void(const LargeSegs&)>& launch_large) {
  const bool bounds = queue_segment_bounds(ctx, segs, A);
  if (bounds) {
    if (!ctx->dm_ev) hipchk(hipEventCreateWithFlags(&ctx->dm_ev, hipEventDisableTiming), "event create");
    hipchk(hipEventRecord(ctx->dm_ev, ctx->stream), "event record");
  }
  launch_units();
  if (!bounds) return;
  hipchk(hipEventSynchronize(ctx->dm_ev), "wait for the segment bounds");
  std::vector<pe::FitLarge> large;
  const int64_t nodes = pe::fit_scratch_layout(plan, ctx->dm_hoff.p, ctx->Ns, pe::PL_LDS_NODES, large);
  if (large.empty()) return;
  const size_t bytes = large.size() * sizeof(pe::FitLarge);
  hipchk(ctx->dm_hlarge.ensure(bytes), "alloc pinned large-segment records");
  hipchk(ctx->dm_large.ensure(bytes), "alloc large-segment records");
  if (ctx->dm_scratch.ensure((size_t)(pe::D * nodes)) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);   // the units already queued touch the call's own buffers only
    raise(PE_ENOMEM, "working copies of the large segments: device allocation failed");
  }
  std::memcpy(ctx->dm_hlarge.p, large.data(), bytes);
  hipchk(hipMemcpyAsync(ctx->dm_large.p, ctx->dm_hlarge.p, bytes, hipMemcpyHostToDevice, ctx->stream),
         "H2D large-segment records");
  launch_large({(const pe::FitLarge*)ctx->dm_large.p, (int64_t)large.size(), ctx->dm_scratch.p});
}

void mirror_follow(pe_ctx* ctx, const char* kernel, int64_t J, const int32_t* job_group_off, const int64_t* group_req,
                   const int64_t* pod_off, const int32_t* pods, const int32_t* status, const int32_t* group_pods,
                   int64_t* out_job_pods) {
  int64_t placed_pods = 0, placed = 0;
  for (int64_t j = 0; j < J; ++j) {
    int64_t job_pods = 0;
    if (status[j] == PE_JOB_PLACED) {
      ++placed;
      for (int64_t g = job_group_off[j]; g < job_group_off[j + 1]; ++g) {
        const int64_t p0 = pod_off[g], p1 = group_pods ? p0 + group_pods[g] : pod_off[g + 1];
        if (p1 < p0 || p1 > pod_off[g + 1])
          raise(PE_EHIP, std::string(kernel) + ": a group's placed pods outside its count");
        const int64_t* q = group_req + g * pe::D;
        job_pods += p1 - p0;
        for (int64_t p = p0; p < p1;) {   // a run of one node at a time
          const int32_t node = pods[p];
          int64_t e = p + 1;
          while (e < p1 && pods[e] == node) ++e;
          if (node < 0 || node >= ctx->n_total) raise(PE_EHIP, std::string(kernel) + ": a placed pod without a node");
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
}

}  // namespace pe_engine
