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
    // ---- one pinned block in: the groups, the pairs in plan order, the units, the records (8-B aligned so far),
    // then the record CSR, the lists and the plan's words
    const size_t pairs_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t units_at = pairs_at + (size_t)P * sizeof(pe::PrePair);
    const size_t recs_at = units_at + (size_t)U * sizeof(pe::FitUnit);
    const size_t rstart_at = recs_at + (size_t)R * sizeof(pe::PreRec);
    const size_t list_at = rstart_at + (size_t)(V + 1) * sizeof(int32_t);
    const size_t words_at = list_at + (size_t)NL * sizeof(int32_t);
    const size_t in_bytes = words_at + (size_t)(L0 + ND) * sizeof(int32_t);
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned gang-preempt inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc gang-preempt inputs");
    fill_place_groups((pe::PlaceGroup*)ctx->dm_hin.p, G, group_req, group_need, group_count, nullptr);
    pe::PrePair* const h_pairs = (pe::PrePair*)(ctx->dm_hin.p + pairs_at);
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = fit.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::PrePair{p, j, job_group_off[j], job_group_off[j + 1], plan.list_start[(size_t)i],
                               plan.list_start[(size_t)i + 1], {0, 0}};
    }
    std::memcpy(ctx->dm_hin.p + units_at, fit.units.data(), (size_t)U * sizeof(pe::FitUnit));
    std::memcpy(ctx->dm_hin.p + recs_at, plan.recs.data(), (size_t)R * sizeof(pe::PreRec));
    std::memcpy(ctx->dm_hin.p + rstart_at, plan.rec_start.data(), (size_t)(V + 1) * sizeof(int32_t));
    std::memcpy(ctx->dm_hin.p + list_at, plan.list.data(), (size_t)NL * sizeof(int32_t));
    pack_domain_words((int32_t*)(ctx->dm_hin.p + words_at), fit.leaf_dom, fit.act_of);
    hipchk(hipMemcpyAsync(ctx->dm_in.p, ctx->dm_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream),
           "H2D gang-preempt inputs");
    const int32_t* const d_words = (const int32_t*)(ctx->dm_in.p + words_at);
    // ---- the call's device buffers; the answers: best [J] and the judgement counter (64-bit cells), then victims,
    // prefix and count [P], 16-B aligned
    const size_t judged_at = (size_t)J * sizeof(uint64_t);
    const size_t vict_at = r16(judged_at + sizeof(uint64_t));
    const size_t prefix_at = vict_at + r16((size_t)P * sizeof(uint64_t));
    const size_t count_at = prefix_at + r16((size_t)P * sizeof(int32_t));
    const size_t out_bytes = count_at + (size_t)P * sizeof(int32_t);
    hipchk(ctx->dm_out.ensure(out_bytes), "alloc gang-preempt outputs");
    hipchk(ctx->pp_place.ensure((size_t)std::max<int64_t>(ctx->Ns, 1)), "alloc node places");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::PreIn in{};
    in.groups = (const pe::PlaceGroup*)ctx->dm_in.p;
    in.pairs = (const pe::PrePair*)(ctx->dm_in.p + pairs_at);
    in.units = (const pe::FitUnit*)(ctx->dm_in.p + units_at);
    in.recs = (const pe::PreRec*)(ctx->dm_in.p + recs_at);
    in.rec_start = (const int32_t*)(ctx->dm_in.p + rstart_at);
    in.list = (const int32_t*)(ctx->dm_in.p + list_at);
    in.node_place = ctx->pp_place.p;
    in.Ns = ctx->Ns;
    in.id_base = (uint64_t)ctx->begin;
    pe::PreOut out{(unsigned long long*)ctx->dm_out.p, (unsigned long long*)(ctx->dm_out.p + judged_at),
                   (uint64_t*)(ctx->dm_out.p + vict_at), (int32_t*)(ctx->dm_out.p + prefix_at),
                   (int32_t*)(ctx->dm_out.p + count_at)};
    hipchk(hipMemsetAsync(out.best, 0xFF, judged_at, ctx->stream), "clear best pairs");
    hipchk(hipMemsetAsync(out.judged, 0, sizeof(uint64_t), ctx->stream), "zero the judgement counter");
    if (ctx->Ns > 0)
      hipchk(hipMemsetAsync(ctx->pp_place.p, 0xFF, (size_t)ctx->Ns * sizeof(int32_t), ctx->stream), "clear node places");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    hipchk(pe::launch_preempt_place_map(ctx->stream, segs, (int)A, ctx->Ns, (uint64_t)ctx->begin, ctx->pp_place.p),
           "launch preempt_place_map");
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_preempt(ctx->stream, in, blocks, large.recs, large.scratch, segs, out), what);
    };
    launch_units_then_large(
        ctx, segs, A, fit, [&]() { launch(U, {}, "launch preempt_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch preempt_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for (the judgement counter
    // lies behind best and crosses with it, or alone for the diagnostics)
    const size_t lo = out_best ? 0 : ev.on ? judged_at : out_victims ? vict_at : out_prefix ? prefix_at : count_at;
    const size_t hi = out_count     ? out_bytes
                      : out_prefix  ? prefix_at + (size_t)P * sizeof(int32_t)
                      : out_victims ? vict_at + (size_t)P * sizeof(uint64_t)
                                    : judged_at + sizeof(uint64_t);
    if (out_best || out_victims || out_prefix || out_count || ev.on) {
      hipchk(ctx->dm_hout.ensure(hi), "alloc pinned gang-preempt outputs");
      hipchk(hipMemcpyAsync(ctx->dm_hout.p + lo, ctx->dm_out.p + lo, hi - lo, hipMemcpyDeviceToHost, ctx->stream),
             "D2H gang-preempt answers");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync gang_preempt_domains");
    const uint8_t* const h = ctx->dm_hout.p;
    if (out_best) {   // the low half of the minimum is the pair; ~0 reads as -1: no pair has an answer
      const uint64_t* const best = (const uint64_t*)h;
      for (int64_t j = 0; j < J; ++j) out_best[j] = (int32_t)(uint32_t)best[j];
    }
    if (out_victims) std::memcpy(out_victims, h + vict_at, (size_t)P * sizeof(uint64_t));
    if (out_prefix) std::memcpy(out_prefix, h + prefix_at, (size_t)P * sizeof(int32_t));
    if (out_count) std::memcpy(out_count, h + count_at, (size_t)P * sizeof(int32_t));
    if (ev.on) {
      uint64_t judged = 0;
      std::memcpy(&judged, h + judged_at, sizeof(judged));
      ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " judged=" + std::to_string(judged));
    }
    return PE_OK;
  });
}

}  // extern "C"
