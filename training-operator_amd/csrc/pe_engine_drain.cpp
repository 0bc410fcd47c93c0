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

}  // namespace

namespace pe_engine {

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

}  // namespace pe_engine

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
    pe::BlockLayout in;
    const auto runs = in.add<pe::PlaceGroup>(R);
    const auto pairs = in.add<pe::DrainPair>(C);
    const auto units = in.add<pe::FitUnit>(U);
    const auto words = in.add<int32_t>(L0 + ND);
    const auto slots = in.add<int32_t>(E);
    uint8_t* const h = block_in_host(ctx, in, "drain-fit");
    for (int64_t r = 0; r < R; ++r) {
      const pe::DrainRun& run = plan.runs[(size_t)r];
      pe::PlaceGroup& o = runs.in(h)[r];
      std::memset(&o, 0, sizeof(o));
      for (int d = 0; d < pe::D; ++d) o.q[d] = group_req[(int64_t)run.group * pe::D + d];
      o.need = group_need ? group_need[run.group] : 0u;
      o.count = run.count;
      o.pod0 = run.pod0;
    }
    pe::DrainPair* const h_pairs = pairs.in(h);
    for (int64_t i = 0; i < C; ++i) {
      const int32_t c = plan.fit.pairs[(size_t)i];
      h_pairs[i] = pe::DrainPair{c, cand_node[c], plan.run_start[(size_t)c], plan.run_start[(size_t)c + 1]};
    }
    std::memcpy(units.in(h), plan.fit.units.data(), units.bytes());
    pack_domain_words(words.in(h), plan.fit.leaf_dom, plan.fit.act_of);
    std::memcpy(slots.in(h), plan.slot_list.data(), slots.bytes());
    const uint8_t* const d = block_in_device(ctx, in, "drain-fit");
    // ---- the call's device buffers; the answers: fits, moved and fail_slot [C], then target [S], 16-B aligned
    const bool store = out_target != nullptr;
    pe::BlockLayout ans;
    const auto fits = ans.add<uint8_t>(C, 16, out_fits != nullptr);
    const auto moved = ans.add<int64_t>(C, 16, out_moved != nullptr);
    const auto fail = ans.add<int64_t>(C, 16, out_fail_slot != nullptr);
    const auto target = ans.add<int32_t>(store ? S : 0, 16, store);
    uint8_t* const o = block_out_device(ctx, ans, "drain-fit");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::DrainOut out{fits.in(o), moved.in(o), fail.in(o), store ? target.in(o) : nullptr};
    if (store) hipchk(hipMemsetAsync(out.target, 0xFF, target.bytes(), ctx->stream), "clear targets");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, words.in(d), L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_drain(ctx->stream, runs.in(d), pairs.in(d), units.in(d), blocks, large.recs, large.scratch,
                              slots.in(d), segs, out, store),
             what);
    };
    launch_units_then_large(
        ctx, segs, A, plan.fit, [&]() { launch(U, {}, "launch drain_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch drain_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const uint8_t* const a = block_read_back(ctx, ans, "drain-fit", "sync drain_fit_domains");
    block_part_to(out_fits, fits, a);
    block_part_to(out_moved, moved, a);
    block_part_to(out_fail_slot, fail, a);
    block_part_to(out_target, target, a);
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U) + " E=" + std::to_string(E));
    return PE_OK;
  });
}

}  // extern "C"
