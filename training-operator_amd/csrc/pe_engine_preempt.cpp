// libplacement: which gangs must go for a gang to fit (pe_gang_preempt_domains).  The host validates the batch,
// the hierarchy, the pairs, the victims and the candidate lists, builds the plan (pe_preempt_plan.h) and checks the
// overflow guard against its mirror; the groups, the pair and unit tables, the lists, the release records and the
// plan's words cross in one pinned block and one copy; pe_place.hip's member kernels gather every active domain's
// nodes into a compact segment, one small kernel maps every node to its place there, and the kernels of
// pe_preempt.hip walk every pair through the two phases, one workgroup per unit of at most PRE_UNIT_PAIRS pairs;
// the answers the caller asked for come back in one copy.  Read-only: the device residuals, the host mirror, the
// reset snapshot, the staged fit-mask state and the stats are not touched.  The host path and the buffers are the
// domain calls' (pe_domain_call.h, pe_ctx.h dm_* and pp_place): nothing of the call is kept between calls.
#include "pe_domain_call.h"
#include "pe_preempt_plan.h"

namespace {

[[noreturn]] void raise_plan(pe::PreemptPlanError e, pe::FitPlanError fe, pe::TreePlanError te, int64_t bad) {
  const std::string at = " at index " + std::to_string(bad);
  switch (e) {
    case pe::PRE_BAD_FIT: raise_fit_plan(fe, te, bad);
    case pe::PRE_BAD_VICTIMS: raise(PE_EINVAL, "n_victims outside [0, 2^31 - 1]");
    case pe::PRE_NO_VIC_OFF: raise(PE_EINVAL, "vic_group_off is NULL");
    case pe::PRE_BAD_VIC_OFF: raise(PE_EINVAL, "vic_group_off: not rising from 0" + at);
    case pe::PRE_NO_VIC_GROUPS: raise(PE_EINVAL, "vic_group_count or vic_group_req is NULL");
    case pe::PRE_BAD_VIC_COUNT: raise(PE_EINVAL, "vic_group_count: negative value" + at);
    case pe::PRE_BAD_VIC_REQ: raise(PE_EINVAL, "vic_group_req: negative value in group" + at);
    case pe::PRE_NO_POD_NODE: raise(PE_EINVAL, "vic_pod_node is NULL");
    case pe::PRE_BAD_POD_NODE: raise(PE_EINVAL, "vic_pod_node: value outside [-1, n_total)" + at);
    case pe::PRE_TOO_MANY: raise(PE_EINVAL, "more than 2^31 - 1 release records");
    case pe::PRE_NO_LIST_OFF: raise(PE_EINVAL, "pair_vic_off is NULL");
    case pe::PRE_BAD_LIST_OFF: raise(PE_EINVAL, "pair_vic_off: not rising from 0" + at);
    case pe::PRE_LONG_LIST: raise(PE_EINVAL, "more than PE_MAX_PAIR_VICTIMS candidate victims for the pair" + at);
    case pe::PRE_NO_LIST: raise(PE_EINVAL, "pair_vic is NULL");
    case pe::PRE_BAD_LIST_VICTIM: raise(PE_EINVAL, "pair_vic: value outside [0, n_victims)" + at);
    default: raise(PE_EINVAL, "pair_vic: the same victim twice in one list" + at);
  }
}

}  // namespace

extern "C" {

int pe_gang_preempt_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                            const int64_t* group_req, const uint32_t* group_need, int64_t n_victims,
                            const int32_t* vic_group_off, const int32_t* vic_group_count, const int64_t* vic_group_req,
                            const int32_t* vic_pod_node, int64_t n_pairs, const int32_t* pair_job,
                            const int32_t* pair_domain, const int32_t* pair_vic_off, const int32_t* pair_vic,
                            int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                            int32_t* out_prefix, uint64_t* out_victims, int32_t* out_count, int32_t* out_best) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_gang_preempt_domains", n_jobs);
    const int64_t G = n_jobs > 0 ? check_gang_groups(n_jobs, job_group_off, group_count, group_req) : 0;
    pe::PreemptPlan plan;
    pe::FitPlanError fe = pe::FIT_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::PreemptPlanError err = pe::preempt_plan_build(
        plan, n_jobs, ctx->n_total, n_victims, vic_group_off, vic_group_count, vic_group_req, vic_pod_node, n_pairs,
        pair_job, pair_domain, pair_vic_off, pair_vic, level, n_levels, level_size, parent, &fe, &te, &bad);
    if (err != pe::PRE_OK) raise_plan(err, fe, te, bad);
    // the overflow guard: the current residual plus everything the call's victims hold on the node, so that no set
    // of releases overflows on the device; a removed slot is in no domain and takes no part
    for (int64_t k = 0; k < plan.n_sums(); ++k) {
      const pe::NodeState& m = ctx->m_nodes[(size_t)plan.sum_node[(size_t)k]];
      if (m.res[0] == pe::NEVER) continue;
      for (int d = 0; d < pe::D; ++d) {
        const uint64_t sum = plan.sum_q[(size_t)k * 4 + d];
        if (sum == UINT64_MAX || (__int128)m.res[d] + (__int128)sum > (__int128)INT64_MAX)
          raise(PE_EINVAL, "overflow: the residual plus the victims' requests exceeds int64 at node " +
                               std::to_string(plan.sum_node[(size_t)k]));
      }
    }
    const pe::FitPlan& fit = plan.fit;
    const int64_t J = n_jobs, P = n_pairs, V = n_victims, A = fit.n_active(), U = fit.n_units();
    if (P == 0) {   // no pair: no answer for any job, and nothing runs
      if (out_best) std::fill(out_best, out_best + J, -1);
      return PE_OK;
    }
    const int64_t L0 = fit.n_leaf, ND = fit.n_dom, R = plan.n_recs(), NL = (int64_t)plan.list.size();
    // ---- one pinned block in: the groups, the pairs in plan order, the units, the records, then the record CSR,
    // the lists and the plan's words
    pe::BlockLayout bl;
    const auto groups = bl.add<pe::PlaceGroup>(G);
    const auto pairs = bl.add<pe::PrePair>(P);
    const auto units = bl.add<pe::FitUnit>(U);
    const auto recs = bl.add<pe::PreRec>(R);
    const auto rstart = bl.add<int32_t>(V + 1);
    const auto list = bl.add<int32_t>(NL);
    const auto words = bl.add<int32_t>(L0 + ND);
    uint8_t* const h = block_in_host(ctx, bl, "gang-preempt");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, nullptr);
    pe::PrePair* const h_pairs = pairs.in(h);
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = fit.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::PrePair{p, j, job_group_off[j], job_group_off[j + 1], plan.list_start[(size_t)i],
                               plan.list_start[(size_t)i + 1], {0, 0}};
    }
    std::memcpy(units.in(h), fit.units.data(), units.bytes());
    std::memcpy(recs.in(h), plan.recs.data(), recs.bytes());
    std::memcpy(rstart.in(h), plan.rec_start.data(), rstart.bytes());
    std::memcpy(list.in(h), plan.list.data(), list.bytes());
    pack_domain_words(words.in(h), fit.leaf_dom, fit.act_of);
    const uint8_t* const d = block_in_device(ctx, bl, "gang-preempt");
    // ---- the call's device buffers; the answers: best [J] and the judgement counter (64-bit cells; it crosses with
    // best, or alone for the diagnostics), then victims, prefix and count [P], 16-B aligned
    CapEvents ev(ctx);
    pe::BlockLayout ans;
    const auto best = ans.add<unsigned long long>(J, 16, out_best != nullptr);
    const auto judged = ans.add<unsigned long long>(1, 8, out_best || ev.on);
    const auto victims = ans.add<uint64_t>(P, 16, out_victims != nullptr);
    const auto prefix = ans.add<int32_t>(P, 16, out_prefix != nullptr);
    const auto count = ans.add<int32_t>(P, 16, out_count != nullptr);
    uint8_t* const o = block_out_device(ctx, ans, "gang-preempt");
    hipchk(ctx->pp_place.ensure((size_t)std::max<int64_t>(ctx->Ns, 1)), "alloc node places");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::PreIn in{};
    in.groups = groups.in(d);
    in.pairs = pairs.in(d);
    in.units = units.in(d);
    in.recs = recs.in(d);
    in.rec_start = rstart.in(d);
    in.list = list.in(d);
    in.node_place = ctx->pp_place.p;
    in.Ns = ctx->Ns;
    in.id_base = (uint64_t)ctx->begin;
    pe::PreOut out{best.in(o), judged.in(o), victims.in(o), prefix.in(o), count.in(o)};
    hipchk(hipMemsetAsync(out.best, 0xFF, best.bytes(), ctx->stream), "clear best pairs");
    hipchk(hipMemsetAsync(out.judged, 0, judged.bytes(), ctx->stream), "zero the judgement counter");
    if (ctx->Ns > 0)
      hipchk(hipMemsetAsync(ctx->pp_place.p, 0xFF, (size_t)ctx->Ns * sizeof(int32_t), ctx->stream), "clear node places");
    ev.begin();
    launch_domain_members(ctx, words.in(d), L0, A, segs);
    hipchk(pe::launch_preempt_place_map(ctx->stream, segs, (int)A, ctx->Ns, (uint64_t)ctx->begin, ctx->pp_place.p),
           "launch preempt_place_map");
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_preempt(ctx->stream, in, blocks, large.recs, large.scratch, segs, out), what);
    };
    launch_units_then_large(
        ctx, segs, A, fit, [&]() { launch(U, {}, "launch preempt_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch preempt_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const uint8_t* const a = block_read_back(ctx, ans, "gang-preempt", "sync gang_preempt_domains");
    block_best_to(out_best, best, a);
    block_part_to(out_victims, victims, a);
    block_part_to(out_prefix, prefix, a);
    block_part_to(out_count, count, a);
    if (ev.on)
      ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " judged=" + std::to_string(*judged.in(a)));
    return PE_OK;
  });
}

}  // extern "C"
