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
    // ---- one pinned block in: the groups, the pairs in plan order, the templates' residuals, the units, then the
    // templates' labels, the new slots and the plan's words
    pe::BlockLayout bl;
    const auto groups = bl.add<pe::PlaceGroup>(G);
    const auto pairs = bl.add<pe::ScalePair>(P);
    const auto tres = bl.add<int64_t>(T * pe::D);
    const auto units = bl.add<pe::FitUnit>(U);
    const auto tlab = bl.add<uint32_t>(T);
    const auto slots = bl.add<int32_t>(n_new);
    const auto words = bl.add<int32_t>(L0 + ND);
    uint8_t* const h = block_in_host(ctx, bl, "scale-up");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, nullptr);
    pe::ScalePair* const h_pairs = pairs.in(h);
    int64_t attempts = 0;   // the judgements the call may cost
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = fit.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::ScalePair{p, j, job_group_off[j], job_group_off[j + 1], pair_template[p], plan.kmax[(size_t)i], {0, 0}};
      attempts += plan.kmax[(size_t)i] + 1;
    }
    std::memcpy(tres.in(h), tmpl_res, tres.bytes());
    std::memcpy(units.in(h), fit.units.data(), units.bytes());
    uint32_t* const h_tlab = tlab.in(h);
    for (int64_t t = 0; t < T; ++t)   // a node in a domain has an island: the caller's bit 31 is replaced
      h_tlab[t] = (tmpl_labels ? tmpl_labels[t] : 0u) | PE_LABEL_ISLAND;
    if (n_new > 0) std::memcpy(slots.in(h), new_slot, slots.bytes());
    pack_domain_words(words.in(h), fit.leaf_dom, fit.act_of);
    const uint8_t* const d = block_in_device(ctx, bl, "scale-up");
    // ---- the call's device buffers; the answers: best [J] (64-bit cells), then nodes, fail_group, pods and new_pods
    // [P], 16-B aligned
    pe::BlockLayout ans;
    const auto best = ans.add<unsigned long long>(J, 16, out_best != nullptr);
    const auto nodes = ans.add<int32_t>(P, 16, out_nodes != nullptr);
    const auto fail = ans.add<int32_t>(P, 16, out_fail_group != nullptr);
    const auto pods = ans.add<int64_t>(P, 16, out_pods != nullptr);
    const auto newp = ans.add<int64_t>(P, 16, out_new_pods != nullptr);
    uint8_t* const o = block_out_device(ctx, ans, "scale-up");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::ScaleIn in{};
    in.groups = groups.in(d);
    in.pairs = pairs.in(d);
    in.units = units.in(d);
    in.tmpl_res = tres.in(d);
    in.tmpl_lab = tlab.in(d);
    in.new_slot = slots.in(d);
    in.n_new = n_new;
    pe::ScaleOut out{best.in(o), nodes.in(o), fail.in(o), pods.in(o), newp.in(o)};
    hipchk(hipMemsetAsync(out.best, 0xFF, best.bytes(), ctx->stream), "clear best pairs");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, words.in(d), L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_scale(ctx->stream, in, blocks, large.recs, large.scratch, segs, out), what);
    };
    launch_units_then_large(
        ctx, segs, A, fit, [&]() { launch(U, {}, "launch scale_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch scale_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const uint8_t* const a = block_read_back(ctx, ans, "scale-up", "sync scale_up_domains");
    block_best_to(out_best, best, a);
    block_part_to(out_nodes, nodes, a);
    block_part_to(out_fail_group, fail, a);
    block_part_to(out_pods, pods, a);
    block_part_to(out_new_pods, newp, a);
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " attempts<=" + std::to_string(attempts));
    return PE_OK;
  });
}

}  // extern "C"
