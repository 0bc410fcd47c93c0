// libplacement: fewest new nodes for a gang to fit a domain (pe_scale_up_domains).  The host validates the batch, the
// hierarchy, the pairs, the templates and the new slots and builds the plan (pe_scale_plan.h: the fit call's plan with
// the work units cut by the attempts a pair may cost); the groups, the pairs in plan order, the templates, the new
// slots, the units and the plan's words cross in one pinned block and one copy; pe_place.hip's member kernels gather
// every active domain's nodes into a compact segment and the kernels of pe_scale.hip walk every pair through its
// attempts in ascending order, one workgroup per unit; the answers the caller asked for come back in one copy.
// Read-only: the device residuals, the host mirror, the reset snapshot, the staged fit-mask state and the stats are
// not touched.  The host path and the buffers are the domain calls' (pe_domain_call.h, pe_ctx.h dm_*): nothing of the
// call is kept between calls.
#include "pe_domain_call.h"
#include "pe_scale_plan.h"

static_assert(pe::SCALE_MAX_NEW == PE_MAX_SCALE_NODES && pe::SCALE_MAX_NODES == PE_MAX_SCALE_NODES, "PE_MAX_SCALE_NODES");

namespace {

[[noreturn]] void raise_scale_plan(pe::ScalePlanError e, pe::FitPlanError fe, pe::TreePlanError te, int64_t bad) {
  const std::string at = " at index " + std::to_string(bad);
  switch (e) {
    case pe::SCALE_BAD_FIT: raise_fit_plan(fe, te, bad);
    case pe::SCALE_BAD_TEMPLATES: raise(PE_EINVAL, "n_templates < 0, or < 1 with pairs");
    case pe::SCALE_NO_TEMPLATES: raise(PE_EINVAL, "tmpl_res is NULL");
    case pe::SCALE_BAD_TMPL_RES: raise(PE_EINVAL, "tmpl_res: negative value in template" + at);
    case pe::SCALE_BAD_NEW: raise(PE_EINVAL, "n_new outside [0, PE_MAX_SCALE_NODES]");
    case pe::SCALE_NO_NEW: raise(PE_EINVAL, "new_slot is NULL");
    case pe::SCALE_BAD_SLOT: raise(PE_EINVAL, "new_slot: value outside [0, n_total)" + at);
    case pe::SCALE_LIVE_SLOT: raise(PE_EINVAL, "new_slot: not a removed slot" + at);
    case pe::SCALE_DUP_SLOT: raise(PE_EINVAL, "new_slot: a slot named twice" + at);
    case pe::SCALE_NO_PAIR_TMPL: raise(PE_EINVAL, "pair_template is NULL");
    case pe::SCALE_BAD_PAIR_TMPL: raise(PE_EINVAL, "pair_template: value outside [0, n_templates)" + at);
    default: raise(PE_EINVAL, "pair_max: value outside [0, n_new]" + at);
  }
}

}  // namespace

extern "C" {

int pe_scale_up_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                        const int64_t* group_req, const uint32_t* group_need, int32_t n_templates,
                        const int64_t* tmpl_res, const uint32_t* tmpl_labels, int32_t n_new, const int32_t* new_slot,
                        int64_t n_pairs, const int32_t* pair_job, const int32_t* pair_domain,
                        const int32_t* pair_template, const int32_t* pair_max, int32_t level, int32_t n_levels,
                        const int32_t* level_size, const int32_t* parent, int32_t* out_nodes, int32_t* out_fail_group,
                        int64_t* out_pods, int64_t* out_new_pods, int32_t* out_best) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_scale_up_domains", n_jobs);
    const int64_t G = n_jobs > 0 ? check_gang_groups(n_jobs, job_group_off, group_count, group_req) : 0;
    pe::ScalePlan plan;
    pe::FitPlanError fe = pe::FIT_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::ScalePlanError err = pe::scale_plan_build(
        plan, n_jobs, ctx->n_total, n_templates, tmpl_res, n_new, new_slot, n_pairs, pair_job, pair_domain,
        pair_template, pair_max, level, n_levels, level_size, parent,
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res[0] == pe::NEVER; }, &fe, &te, &bad);
    if (err != pe::SCALE_OK) raise_scale_plan(err, fe, te, bad);
    const pe::FitPlan& fit = plan.fit;
    const int64_t J = n_jobs, P = n_pairs, T = n_templates, A = fit.n_active(), U = fit.n_units();
    if (P == 0) {   // no pair: no answer for any job, and nothing runs
      if (out_best) std::fill(out_best, out_best + J, -1);
      return PE_OK;
    }
    const int64_t L0 = fit.n_leaf, ND = fit.n_dom;
    // ---- one pinned block in: the groups, the pairs in plan order, the templates' residuals (8-B aligned so far),
    // the units, then the templates' labels, the new slots and the plan's words
    const size_t pairs_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t tres_at = pairs_at + (size_t)P * sizeof(pe::ScalePair);
    const size_t units_at = tres_at + (size_t)T * pe::D * sizeof(int64_t);
    const size_t tlab_at = units_at + (size_t)U * sizeof(pe::FitUnit);
    const size_t slots_at = tlab_at + (size_t)T * sizeof(uint32_t);
    const size_t words_at = slots_at + (size_t)n_new * sizeof(int32_t);
    const size_t in_bytes = words_at + (size_t)(L0 + ND) * sizeof(int32_t);
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned scale-up inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc scale-up inputs");
    fill_place_groups((pe::PlaceGroup*)ctx->dm_hin.p, G, group_req, group_need, group_count, nullptr);
    pe::ScalePair* const h_pairs = (pe::ScalePair*)(ctx->dm_hin.p + pairs_at);
    int64_t attempts = 0;   // the judgements the call may cost
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = fit.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::ScalePair{p, j, job_group_off[j], job_group_off[j + 1], pair_template[p], plan.kmax[(size_t)i], {0, 0}};
      attempts += plan.kmax[(size_t)i] + 1;
    }
    std::memcpy(ctx->dm_hin.p + tres_at, tmpl_res, (size_t)T * pe::D * sizeof(int64_t));
    std::memcpy(ctx->dm_hin.p + units_at, fit.units.data(), (size_t)U * sizeof(pe::FitUnit));
    uint32_t* const h_tlab = (uint32_t*)(ctx->dm_hin.p + tlab_at);
    for (int64_t t = 0; t < T; ++t)   // a node in a domain has an island: the caller's bit 31 is replaced
      h_tlab[t] = (tmpl_labels ? tmpl_labels[t] : 0u) | PE_LABEL_ISLAND;
    if (n_new > 0) std::memcpy(ctx->dm_hin.p + slots_at, new_slot, (size_t)n_new * sizeof(int32_t));
    pack_domain_words((int32_t*)(ctx->dm_hin.p + words_at), fit.leaf_dom, fit.act_of);
    hipchk(hipMemcpyAsync(ctx->dm_in.p, ctx->dm_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D scale-up inputs");
    const int32_t* const d_words = (const int32_t*)(ctx->dm_in.p + words_at);
    // ---- the call's device buffers; the answers: best [J] (64-bit cells), then nodes, fail_group, pods and new_pods
    // [P], 16-B aligned
    const size_t nodes_at = r16((size_t)J * sizeof(uint64_t));
    const size_t fail_at = nodes_at + r16((size_t)P * sizeof(int32_t));
    const size_t pods_at = fail_at + r16((size_t)P * sizeof(int32_t));
    const size_t newp_at = pods_at + r16((size_t)P * sizeof(int64_t));
    const size_t out_bytes = newp_at + (size_t)P * sizeof(int64_t);
    hipchk(ctx->dm_out.ensure(out_bytes), "alloc scale-up outputs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::ScaleIn in{};
    in.groups = (const pe::PlaceGroup*)ctx->dm_in.p;
    in.pairs = (const pe::ScalePair*)(ctx->dm_in.p + pairs_at);
    in.units = (const pe::FitUnit*)(ctx->dm_in.p + units_at);
    in.tmpl_res = (const int64_t*)(ctx->dm_in.p + tres_at);
    in.tmpl_lab = (const uint32_t*)(ctx->dm_in.p + tlab_at);
    in.new_slot = (const int32_t*)(ctx->dm_in.p + slots_at);
    in.n_new = n_new;
    pe::ScaleOut out{(unsigned long long*)ctx->dm_out.p, (int32_t*)(ctx->dm_out.p + nodes_at),
                     (int32_t*)(ctx->dm_out.p + fail_at), (int64_t*)(ctx->dm_out.p + pods_at),
                     (int64_t*)(ctx->dm_out.p + newp_at)};
    hipchk(hipMemsetAsync(out.best, 0xFF, (size_t)J * sizeof(uint64_t), ctx->stream), "clear best pairs");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_scale(ctx->stream, in, blocks, large.recs, large.scratch, segs, out), what);
    };
    launch_units_then_large(
        ctx, segs, A, fit, [&]() { launch(U, {}, "launch scale_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch scale_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const size_t lo = out_best ? 0 : out_nodes ? nodes_at : out_fail_group ? fail_at : out_pods ? pods_at : newp_at;
    const size_t hi = out_new_pods     ? out_bytes
                      : out_pods       ? pods_at + (size_t)P * sizeof(int64_t)
                      : out_fail_group ? fail_at + (size_t)P * sizeof(int32_t)
                      : out_nodes      ? nodes_at + (size_t)P * sizeof(int32_t)
                                       : (size_t)J * sizeof(uint64_t);
    if (out_best || out_nodes || out_fail_group || out_pods || out_new_pods) {
      hipchk(ctx->dm_hout.ensure(hi), "alloc pinned scale-up outputs");
      hipchk(hipMemcpyAsync(ctx->dm_hout.p + lo, ctx->dm_out.p + lo, hi - lo, hipMemcpyDeviceToHost, ctx->stream),
             "D2H scale-up answers");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync scale_up_domains");
    const uint8_t* const h = ctx->dm_hout.p;
    if (out_best) {   // the low half of the minimum is the pair; ~0 reads as -1: no pair has an answer
      const uint64_t* const best = (const uint64_t*)h;
      for (int64_t j = 0; j < J; ++j) out_best[j] = (int32_t)(uint32_t)best[j];
    }
    if (out_nodes) std::memcpy(out_nodes, h + nodes_at, (size_t)P * sizeof(int32_t));
    if (out_fail_group) std::memcpy(out_fail_group, h + fail_at, (size_t)P * sizeof(int32_t));
    if (out_pods) std::memcpy(out_pods, h + pods_at, (size_t)P * sizeof(int64_t));
    if (out_new_pods) std::memcpy(out_new_pods, h + newp_at, (size_t)P * sizeof(int64_t));
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " attempts<=" + std::to_string(attempts));
    return PE_OK;
  });
}

}  // extern "C"
