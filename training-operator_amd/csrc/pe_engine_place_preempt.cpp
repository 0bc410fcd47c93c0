// libplacement: place a batch, evicting as it goes (pe_place_preempt_domains).  pe_place_greedy_domains' host path
// on the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*) with pe_gang_preempt_domains' victims: the host
// validates the batch, the hierarchy, the victims, the lists and the flags, builds the plan
// (pe_place_preempt_plan.h) and checks the release bound against its mirror and the reset snapshot; the groups, the
// job records, the release records, the lists and the plan's words cross in one pinned block and one copy; the
// member kernels of pe_place.hip gather every active domain's nodes into a compact segment, pe_preempt.hip's map
// gives every node its place there, the two instances of pe_place_preempt.hip run each domain's jobs and the sweep
// gives the evicted gangs' pods outside their domain back; every answer comes back in one copy.  The host mirror
// follows from that answer: the placements come off (mirror_follow) and ALL the pods of every evicted victim go
// back -- unless the call is a dry run, which leaves the device residuals, the mirror and the stats as they were.
#include "pe_domain_call.h"
#include "pe_place_preempt_plan.h"

namespace {

[[noreturn]] void raise_victims(pe::PreemptPlanError e, int64_t bad) {
  const std::string at = " at index " + std::to_string(bad);
  switch (e) {
    case pe::PRE_BAD_FIT: raise(PE_EINVAL, "n_jobs above 2^31 - 2");
    case pe::PRE_BAD_VICTIMS: raise(PE_EINVAL, "n_victims outside [0, 2^31 - 1]");
    case pe::PRE_NO_VIC_OFF: raise(PE_EINVAL, "vic_group_off is NULL");
    case pe::PRE_BAD_VIC_OFF: raise(PE_EINVAL, "vic_group_off: not rising from 0" + at);
    case pe::PRE_NO_VIC_GROUPS: raise(PE_EINVAL, "vic_group_count or vic_group_req is NULL");
    case pe::PRE_BAD_VIC_COUNT: raise(PE_EINVAL, "vic_group_count: negative value" + at);
    case pe::PRE_BAD_VIC_REQ: raise(PE_EINVAL, "vic_group_req: negative value in group" + at);
    case pe::PRE_NO_POD_NODE: raise(PE_EINVAL, "vic_pod_node is NULL");
    case pe::PRE_BAD_POD_NODE: raise(PE_EINVAL, "vic_pod_node: value outside [-1, n_total)" + at);
    case pe::PRE_TOO_MANY: raise(PE_EINVAL, "more than 2^31 - 1 release records");
    case pe::PRE_NO_LIST_OFF: raise(PE_EINVAL, "job_vic_off is NULL");
    case pe::PRE_BAD_LIST_OFF: raise(PE_EINVAL, "job_vic_off: not rising from 0" + at);
    case pe::PRE_LONG_LIST: raise(PE_EINVAL, "more than PE_MAX_PAIR_VICTIMS candidate victims for the job" + at);
    case pe::PRE_NO_LIST: raise(PE_EINVAL, "job_vic is NULL");
    case pe::PRE_BAD_LIST_VICTIM: raise(PE_EINVAL, "job_vic: value outside [0, n_victims)" + at);
    default: raise(PE_EINVAL, "job_vic: the same victim twice in one list" + at);
  }
}

}  // namespace

extern "C" {

int pe_place_preempt_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                             const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                             const int32_t* job_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                             const int32_t* parent, int64_t n_victims, const int32_t* vic_group_off,
                             const int32_t* vic_group_count, const int64_t* vic_group_req, const int32_t* vic_pod_node,
                             const int32_t* job_vic_off, const int32_t* job_vic, uint32_t flags, int32_t* out_pod_node,
                             int32_t* out_job_status, int32_t* out_job_prefix, uint64_t* out_job_victims,
                             int32_t* out_vic_job) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_place_preempt_domains", n_jobs);
    const int64_t G =
        n_jobs > 0 ? check_place_batch(n_jobs, job_group_off, priority, group_count, group_req, out_pod_node, out_job_status)
                   : 0;
    pe::PlacePreemptPlan pp;
    pe::PlacePlanError be = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    pe::PreemptPlanError ve = pe::PRE_OK;
    int64_t bad = -1;
    switch (pe::place_preempt_plan_build(
        pp, ctx->ld_plan, n_jobs, job_group_off, priority, group_count, job_domain, level, n_levels, level_size, parent,
        ctx->n_total, n_victims, vic_group_off, vic_group_count, vic_group_req, vic_pod_node, job_vic_off, job_vic, flags,
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res; }, [ctx](int32_t n) { return ctx->m_nodes0[(size_t)n].res; },
        &be, &te, &ve, &bad)) {
      case pe::PP_OK: break;
      case pe::PP_BAD_PLACE: raise_place_plan(be, te, bad);
      case pe::PP_BAD_VICTIMS: raise_victims(ve, bad);
      case pe::PP_TWO_DOMAINS:
        raise(PE_EINVAL, "job_vic: a victim in the lists of jobs of two domains at index " + std::to_string(bad));
      case pe::PP_BAD_FLAGS: raise(PE_EINVAL, "flags: unknown bits");
      case pe::PP_OVER:
        raise(PE_EINVAL, "pe_place_preempt_domains: the victims give back more than was taken (the residual would exceed "
                         "the reset snapshot) at node " + std::to_string(bad));
    }
    const int64_t J = n_jobs, V = n_victims;
    if (J == 0) {   // nobody evicts anybody
      if (out_vic_job) std::fill(out_vic_job, out_vic_job + V, -1);
      return PE_OK;
    }
    const pe::PlacePlan& plan = pp.base;
    const int64_t A = plan.n_active(), P = plan.pods(), L0 = plan.n_leaf, ND = plan.n_dom, R = pp.n_recs();
    const int64_t NL = job_vic_off[J];
    // ---- one pinned block in: the groups, the records, the jobs in plan order, then the record CSR, the victims'
    // active domains, the lists and the plan's words with job_start behind them
    pe::BlockLayout bl;
    const auto groups = bl.add<pe::PlaceGroup>(G);
    const auto recs = bl.add<pe::PreRec>(R);
    const auto jobs = bl.add<pe::PreemptJob>(J);
    const auto rstart = bl.add<int32_t>(V + 1);
    const auto act = bl.add<int32_t>(V);
    const auto list = bl.add<int32_t>(NL);
    const auto words = bl.add<int32_t>(L0 + ND + A + 1);
    uint8_t* const h = block_in_host(ctx, bl, "place-preempt");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, plan.pod_off.data());
    if (R > 0) std::memcpy(recs.in(h), pp.recs.data(), recs.bytes());
    std::memcpy(jobs.in(h), pp.jobs.data(), jobs.bytes());
    std::memcpy(rstart.in(h), pp.rec_start.data(), rstart.bytes());
    if (V > 0) std::memcpy(act.in(h), pp.vic_act.data(), act.bytes());
    if (NL > 0) std::memcpy(list.in(h), job_vic, list.bytes());
    int32_t* const h_start = pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    std::memcpy(h_start, plan.job_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    const uint8_t* const d = block_in_device(ctx, bl, "place-preempt");
    const int32_t* const d_words = words.in(d);
    // ---- one block out: the masks [J] and the attempt counter (64-bit cells), then pods [P], statuses and prefixes
    // [J] and the evicting jobs [V]
    pe::BlockLayout ans;
    const auto masks = ans.add<uint64_t>(J, 8, true);
    const auto tries = ans.add<unsigned long long>(1, 8, true);
    const auto pods = ans.add<int32_t>(P, 4, true);
    const auto status = ans.add<int32_t>(J, 4, true);
    const auto prefix = ans.add<int32_t>(J, 4, true);
    const auto vjob = ans.add<int32_t>(V, 4, true);
    uint8_t* const o = block_out_device(ctx, ans, "place-preempt", true);
    hipchk(ctx->dm_log.ensure((size_t)(3 * P)), "alloc placement logs");
    hipchk(ctx->pp_place.ensure((size_t)std::max<int64_t>(ctx->Ns, 1)), "alloc node places");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::PlacePreIn in{};
    in.groups = groups.in(d);
    in.jobs = jobs.in(d);
    in.job_start = d_words + L0 + ND;
    in.list = list.in(d);
    in.rec_start = rstart.in(d);
    in.recs = recs.in(d);
    in.vic_act = act.in(d);
    in.node_place = ctx->pp_place.p;
    in.Ns = ctx->Ns;
    in.id_base = (uint64_t)ctx->begin;
    const pe::PlacePreOut out{pods.in(o), status.in(o), prefix.in(o), masks.in(o), vjob.in(o), tries.in(o)};
    hipchk(hipMemsetAsync(out.attempts, 0, tries.bytes(), ctx->stream), "zero the attempt counter");
    if (V > 0) hipchk(hipMemsetAsync(out.vic_job, 0xFF, vjob.bytes(), ctx->stream), "clear evicting jobs");
    if (ctx->Ns > 0)
      hipchk(hipMemsetAsync(ctx->pp_place.p, 0xFF, (size_t)ctx->Ns * sizeof(int32_t), ctx->stream), "clear node places");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(pe::launch_preempt_place_map(ctx->stream, segs, (int)A, ctx->Ns, (uint64_t)ctx->begin, ctx->pp_place.p),
           "launch preempt_place_map");
    hipchk(pe::launch_place_preempt(ctx->stream, in, (int)A, segs, ctx->res.p, ctx->stride, pp.dry_run, out, ctx->dm_log.p),
           "launch place_preempt");
    if (!pp.dry_run)
      hipchk(pe::launch_place_preempt_sweep(ctx->stream, in, V, segs, out.vic_job, ctx->res.p, ctx->stride),
             "launch place_preempt_sweep");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "place-preempt", "sync place_preempt_domains");
    block_part_to(out_pod_node, pods, a);
    block_part_to(out_job_status, status, a);
    block_part_to(out_job_prefix, prefix, a);
    block_part_to(out_job_victims, masks, a);
    block_part_to(out_vic_job, vjob, a);
    const int32_t* const evictor = vjob.in(a);
    int64_t evicted = 0;
    for (int64_t v = 0; v < V; ++v) {
      if (evictor[v] < 0) continue;
      if (evictor[v] >= J || pp.vic_act[(size_t)v] < 0) raise(PE_EHIP, "place_preempt_kernel: a victim evicted by no job");
      ++evicted;
      if (pp.dry_run) continue;
      for (int32_t r = pp.rec_start[(size_t)v]; r < pp.rec_start[(size_t)v + 1]; ++r) {   // the gang leaves whole
        const pe::PreRec& rec = pp.recs[(size_t)r];
        pe::NodeState& m = ctx->m_nodes[(size_t)rec.node];
        if (m.res[0] == pe::NEVER) continue;
        for (int dd = 0; dd < pe::D; ++dd) m.res[dd] += rec.q[dd];
      }
    }
    if (!pp.dry_run)
      mirror_follow(ctx, "place_preempt_kernel", J, job_group_off, group_req, plan.pod_off.data(), pods.in(a),
                    status.in(a));
    if (ev.on)
      ev.report_as("A=" + std::to_string(A) + " attempts=" + std::to_string(*tries.in(a)) +
                   " evicted=" + std::to_string(evicted));
    return PE_OK;
  });
}

}  // extern "C"
