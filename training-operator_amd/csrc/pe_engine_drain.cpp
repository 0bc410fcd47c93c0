// libplacement: can a node's pods move elsewhere, and where (pe_drain_fit_domains).  The host validates the book of
// placed gangs, the candidates and the hierarchy and builds the plan (pe_drain_plan.h): every candidate's evicted
// slots, their runs as the groups of one synthetic job, and the fit call's plan over (candidate, target domain).
// The runs, the candidate and unit tables, the plan's words and the slot lists cross in one pinned block and one
// copy; pe_place.hip's member kernels gather every active domain's nodes into a compact segment and the kernels of
// pe_drain.hip judge every candidate on a private copy of its segment without its own node, one workgroup per unit
// of at most FIT_UNIT_PAIRS candidates; the answers the caller asked for come back in one copy.  Read-only: the
// device residuals, the host mirror, the reset snapshot, the staged fit-mask state and the stats are not touched.
// The host path and the buffers are the domain calls' (pe_domain_call.h, pe_ctx.h dm_*).
#include "pe_domain_call.h"

namespace {

[[noreturn]] void raise_book(pe::GangSlotsError e, int64_t bad) {
  const std::string at = " at index " + std::to_string(bad);
  switch (e) {
    case pe::GANGS_BAD_COUNT: raise(PE_EINVAL, "n_gangs outside [0, 2^31 - 1]");
    case pe::GANGS_NO_OFF: raise(PE_EINVAL, "gang_group_off is NULL");
    case pe::GANGS_BAD_OFF: raise(PE_EINVAL, "gang_group_off: not rising from 0" + at);
    case pe::GANGS_NO_GROUPS: raise(PE_EINVAL, "group_count or group_req is NULL");
    case pe::GANGS_BAD_GROUP_COUNT: raise(PE_EINVAL, "group_count: negative value" + at);
    case pe::GANGS_BAD_REQ: raise(PE_EINVAL, "group_req: negative value in group" + at);
    case pe::GANGS_NO_POD_NODE: raise(PE_EINVAL, "pod_node is NULL");
    default: raise(PE_EINVAL, "pod_node: value outside [-1, n_total)" + at);
  }
}

[[noreturn]] void raise_drain_plan(pe::DrainPlanError e, pe::GangSlotsError ge, pe::FitPlanError fe, pe::TreePlanError te,
                                   int64_t bad) {
  const std::string at = " at index " + std::to_string(bad);
  switch (e) {
    case pe::DRAIN_BAD_GANGS: raise_book(ge, bad);
    case pe::DRAIN_BAD_SLOTS: raise(PE_EINVAL, "more than 2^31 - 1 pod slots");
    case pe::DRAIN_BAD_COUNT: raise(PE_EINVAL, "n_cands outside [0, 2^31 - 1)");
    case pe::DRAIN_NO_CANDS: raise(PE_EINVAL, "cand_node or cand_domain is NULL");
    case pe::DRAIN_BAD_NODE: raise(PE_EINVAL, "cand_node: value outside [0, n_total)" + at);
    case pe::DRAIN_DUP_NODE: raise(PE_EINVAL, "cand_node: a node named twice" + at);
    default:
      if (fe == pe::FIT_BAD_DOMAIN) raise(PE_EINVAL, "cand_domain: value outside [0, level_size[level])" + at);
      raise_fit_plan(fe, te, bad);
  }
}

}  // namespace

extern "C" {

int pe_drain_fit_domains(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off, const int32_t* group_count,
                         const int64_t* group_req, const uint32_t* group_need, const int32_t* pod_node, int64_t n_cands,
                         const int32_t* cand_node, const int32_t* cand_domain, int32_t level, int32_t n_levels,
                         const int32_t* level_size, const int32_t* parent, uint8_t* out_fits, int64_t* out_moved,
                         int64_t* out_fail_slot, int32_t* out_target) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_drain_fit_domains", 0);
    pe::GangSlotsError ge = pe::GANGS_OK;
    pe::FitPlanError fe = pe::FIT_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::DrainPlanError err = pe::drain_plan_build(
        ctx->dr_plan, ctx->n_total, n_gangs, gang_group_off, group_count, group_req, pod_node, n_cands, cand_node,
        cand_domain, level, n_levels, level_size, parent,
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res[0] == pe::NEVER; }, &ge, &fe, &te, &bad);
    if (err != pe::DRAIN_OK) raise_drain_plan(err, ge, fe, te, bad);
    const pe::DrainPlan& plan = ctx->dr_plan;
    const int64_t C = n_cands, S = plan.slots, E = plan.n_evicted(), R = plan.n_runs();
    const int64_t A = plan.fit.n_active(), U = plan.fit.n_units();
    if (E == 0) {   // no pod sits on a candidate: each of them fits with 0 pods, and nothing runs
      if (out_fits) std::fill(out_fits, out_fits + C, (uint8_t)1);
      if (out_moved) std::fill(out_moved, out_moved + C, (int64_t)0);
      if (out_fail_slot) std::fill(out_fail_slot, out_fail_slot + C, (int64_t)-1);
      if (out_target) std::fill(out_target, out_target + S, (int32_t)-1);
      return PE_OK;
    }
    const int64_t L0 = plan.fit.n_leaf, ND = plan.fit.n_dom;
    // ---- one pinned block in: the runs, the candidates in plan order, the units, the plan's words, the slot lists
    const size_t pairs_at = (size_t)R * sizeof(pe::PlaceGroup);
    const size_t units_at = pairs_at + (size_t)C * sizeof(pe::DrainPair);
    const size_t words_at = units_at + (size_t)U * sizeof(pe::FitUnit);
    const size_t slots_at = words_at + (size_t)(L0 + ND) * sizeof(int32_t);
    const size_t in_bytes = slots_at + (size_t)E * sizeof(int32_t);
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned drain-fit inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc drain-fit inputs");
    pe::PlaceGroup* const h_runs = (pe::PlaceGroup*)ctx->dm_hin.p;
    for (int64_t r = 0; r < R; ++r) {
      const pe::DrainRun& run = plan.runs[(size_t)r];
      pe::PlaceGroup& o = h_runs[r];
      std::memset(&o, 0, sizeof(o));
      for (int d = 0; d < pe::D; ++d) o.q[d] = group_req[(int64_t)run.group * pe::D + d];
      o.need = group_need ? group_need[run.group] : 0u;
      o.count = run.count;
      o.pod0 = run.pod0;
    }
    pe::DrainPair* const h_pairs = (pe::DrainPair*)(ctx->dm_hin.p + pairs_at);
    for (int64_t i = 0; i < C; ++i) {
      const int32_t c = plan.fit.pairs[(size_t)i];
      h_pairs[i] = pe::DrainPair{c, cand_node[c], plan.run_start[(size_t)c], plan.run_start[(size_t)c + 1]};
    }
    std::memcpy(ctx->dm_hin.p + units_at, plan.fit.units.data(), (size_t)U * sizeof(pe::FitUnit));
    pack_domain_words((int32_t*)(ctx->dm_hin.p + words_at), plan.fit.leaf_dom, plan.fit.act_of);
    std::memcpy(ctx->dm_hin.p + slots_at, plan.slot_list.data(), (size_t)E * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->dm_in.p, ctx->dm_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D drain-fit inputs");
    const pe::PlaceGroup* const d_runs = (const pe::PlaceGroup*)ctx->dm_in.p;
    const pe::DrainPair* const d_pairs = (const pe::DrainPair*)(ctx->dm_in.p + pairs_at);
    const pe::FitUnit* const d_units = (const pe::FitUnit*)(ctx->dm_in.p + units_at);
    const int32_t* const d_words = (const int32_t*)(ctx->dm_in.p + words_at);
    const int32_t* const d_slots = (const int32_t*)(ctx->dm_in.p + slots_at);
    // ---- the call's device buffers; the answers: fits, moved and fail_slot [C], then target [S], 16-B aligned
    const bool store = out_target != nullptr;
    const size_t moved_at = r16((size_t)C);
    const size_t fail_at = moved_at + r16((size_t)C * sizeof(int64_t));
    const size_t target_at = fail_at + r16((size_t)C * sizeof(int64_t));
    const size_t out_bytes = target_at + (store ? (size_t)S * sizeof(int32_t) : 0);
    hipchk(ctx->dm_out.ensure(out_bytes), "alloc drain-fit outputs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::DrainOut out{ctx->dm_out.p, (int64_t*)(ctx->dm_out.p + moved_at), (int64_t*)(ctx->dm_out.p + fail_at),
                     store ? (int32_t*)(ctx->dm_out.p + target_at) : nullptr};
    if (store) hipchk(hipMemsetAsync(out.target, 0xFF, (size_t)S * sizeof(int32_t), ctx->stream), "clear targets");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_drain(ctx->stream, d_runs, d_pairs, d_units, blocks, large.recs, large.scratch, d_slots, segs, out,
                              store),
             what);
    };
    launch_units_then_large(
        ctx, segs, A, plan.fit, [&]() { launch(U, {}, "launch drain_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch drain_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const size_t lo = out_fits ? 0 : out_moved ? moved_at : out_fail_slot ? fail_at : target_at;
    const size_t hi = out_target      ? out_bytes
                      : out_fail_slot ? fail_at + (size_t)C * sizeof(int64_t)
                      : out_moved     ? moved_at + (size_t)C * sizeof(int64_t)
                                      : (size_t)C;
    if (out_fits || out_moved || out_fail_slot || out_target) {
      hipchk(ctx->dm_hout.ensure(hi), "alloc pinned drain-fit outputs");
      hipchk(hipMemcpyAsync(ctx->dm_hout.p + lo, ctx->dm_out.p + lo, hi - lo, hipMemcpyDeviceToHost, ctx->stream),
             "D2H drain-fit answers");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync drain_fit_domains");
    const uint8_t* const h = ctx->dm_hout.p;
    if (out_fits) std::memcpy(out_fits, h, (size_t)C);
    if (out_moved) std::memcpy(out_moved, h + moved_at, (size_t)C * sizeof(int64_t));
    if (out_fail_slot) std::memcpy(out_fail_slot, h + fail_at, (size_t)C * sizeof(int64_t));
    if (out_target) std::memcpy(out_target, h + target_at, (size_t)S * sizeof(int32_t));
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " E=" + std::to_string(E));
    return PE_OK;
  });
}

}  // extern "C"
