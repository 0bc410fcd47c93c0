// libplacement: drain a batch of nodes, moving as it goes (pe_drain_move_domains).  pe_drain_fit_domains' host path
// on the domain calls' scaffold (pe_domain_call.h, pe_ctx.h dm_*) with a committing end: the host validates the book,
// the candidates, the hierarchy and the flags, builds the plan (pe_drain_move_plan.h) and checks the release bound
// against its mirror and the reset snapshot; the runs, the candidates in plan order, the plan's words with the
// candidates' CSR behind them, the slot list and the two maps of the sweep cross in one pinned block and one copy;
// the member kernels of pe_place.hip gather every active domain's nodes into a compact segment, the bitmap kernel
// cordons the candidates, the two instances of pe_drain_move.hip run each domain's candidates in order and the sweep
// scatters the targets and gives the drained nodes their pods' requests back; every answer comes back in one copy.
// The host mirror follows from that answer: the takes come off (mirror_follow) and the evicted pods of every
// candidate that fits go back to its node -- unless the call is a dry run, which leaves the device residuals and
// the mirror as they were.  pe_stats is left alone either way, as by the ledger calls: a move places nothing new.
#include "pe_domain_call.h"
#include "pe_drain_move_plan.h"

extern "C" {

int pe_drain_move_domains(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off, const int32_t* group_count,
                          const int64_t* group_req, const uint32_t* group_need, const int32_t* pod_node, int64_t n_cands,
                          const int32_t* cand_node, const int32_t* cand_domain, int32_t level, int32_t n_levels,
                          const int32_t* level_size, const int32_t* parent, uint32_t flags, uint8_t* out_fits,
                          int64_t* out_moved, int64_t* out_fail_slot, int32_t* out_target) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_drain_move_domains", 0);
    pe::DrainMovePlan mv;
    pe::DrainPlanError de = pe::DRAIN_OK;
    pe::GangSlotsError ge = pe::GANGS_OK;
    pe::FitPlanError fe = pe::FIT_OK;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    switch (pe::drain_move_plan_build(
        ctx->dr_plan, mv, ctx->ld_plan, ctx->n_total, n_gangs, gang_group_off, group_count, group_req, pod_node, n_cands,
        cand_node, cand_domain, level, n_levels, level_size, parent, flags,
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res[0] == pe::NEVER; },
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res; }, [ctx](int32_t n) { return ctx->m_nodes0[(size_t)n].res; },
        &de, &ge, &fe, &te, &bad)) {
      case pe::DM_OK: break;
      case pe::DM_BAD_DRAIN: raise_drain_plan(de, ge, fe, te, bad);
      case pe::DM_BAD_FLAGS: raise(PE_EINVAL, "flags: unknown bits");
      case pe::DM_OVER:
        raise(PE_EINVAL, "pe_drain_move_domains: the candidates' pods give back more than was taken (the residual would "
                         "exceed the reset snapshot) at node " + std::to_string(bad));
    }
    const pe::DrainPlan& plan = ctx->dr_plan;
    const int64_t C = n_cands, S = plan.slots, E = plan.n_evicted(), R = plan.n_runs(), A = plan.fit.n_active();
    if (E == 0) {   // no pod sits on a candidate: each of them fits with 0 pods, nothing moves and nothing runs
      if (out_fits) std::fill(out_fits, out_fits + C, (uint8_t)1);
      if (out_moved) std::fill(out_moved, out_moved + C, (int64_t)0);
      if (out_fail_slot) std::fill(out_fail_slot, out_fail_slot + C, (int64_t)-1);
      if (out_target) std::fill(out_target, out_target + S, (int32_t)-1);
      return PE_OK;
    }
    const int64_t L0 = plan.fit.n_leaf, ND = plan.fit.n_dom;
    // ---- one pinned block in: the runs, the candidates in plan order, the plan's words with the candidates' CSR
    // behind them, the slot list, every place's run and every run's candidate (its place in plan order)
    pe::BlockLayout in;
    const auto runs = in.add<pe::PlaceGroup>(R);
    const auto pairs = in.add<pe::DrainPair>(C);
    const auto words = in.add<int32_t>(L0 + ND + A + 1);
    const auto slots = in.add<int32_t>(E);
    const auto run_of = in.add<int32_t>(E);
    const auto run_pair = in.add<int32_t>(R);
    uint8_t* const h = block_in_host(ctx, in, "drain-move");
    std::vector<int64_t> run_req((size_t)R * pe::D), pod_off((size_t)R + 1);   // the mirror's view of the runs
    for (int64_t r = 0; r < R; ++r) {
      const pe::DrainRun& run = plan.runs[(size_t)r];
      pe::PlaceGroup& o = runs.in(h)[r];
      std::memset(&o, 0, sizeof(o));
      for (int d = 0; d < pe::D; ++d) o.q[d] = run_req[(size_t)(r * pe::D + d)] = group_req[(int64_t)run.group * pe::D + d];
      o.need = group_need ? group_need[run.group] : 0u;
      o.count = run.count;
      o.pod0 = pod_off[(size_t)r] = run.pod0;
      std::fill(run_of.in(h) + run.pod0, run_of.in(h) + run.pod0 + run.count, (int32_t)r);
    }
    pod_off[(size_t)R] = E;
    pe::DrainPair* const h_pairs = pairs.in(h);
    for (int64_t i = 0; i < C; ++i) {
      const int32_t c = plan.fit.pairs[(size_t)i];
      h_pairs[i] = pe::DrainPair{c, cand_node[c], plan.run_start[(size_t)c], plan.run_start[(size_t)c + 1]};
      std::fill(run_pair.in(h) + h_pairs[i].g0, run_pair.in(h) + h_pairs[i].g1, (int32_t)i);
    }
    int32_t* const h_start = pack_domain_words(words.in(h), plan.fit.leaf_dom, plan.fit.act_of);
    std::memcpy(h_start, plan.fit.pair_start.data(), (size_t)(A + 1) * sizeof(int32_t));
    std::memcpy(slots.in(h), plan.slot_list.data(), slots.bytes());
    const uint8_t* const d = block_in_device(ctx, in, "drain-move");
    // ---- one block out: fits, moved and fail_slot [C], the node of every place of the slot list [E], target [S].
    // The host follows the takes from fits and the places, so they cross for every committed call
    const bool dry = mv.dry_run, store = out_target != nullptr;
    pe::BlockLayout ans;
    const auto fits = ans.add<uint8_t>(C, 16, out_fits != nullptr || !dry);
    const auto moved = ans.add<int64_t>(C, 16, out_moved != nullptr);
    const auto fail = ans.add<int64_t>(C, 16, out_fail_slot != nullptr);
    const auto row = ans.add<int32_t>(E, 16, !dry);
    const auto target = ans.add<int32_t>(store ? S : 0, 16, store);
    uint8_t* const o = block_out_device(ctx, ans, "drain-move");
    hipchk(ctx->dm_log.ensure((size_t)(3 * E)), "alloc move logs");
    const size_t cordon_words = ((size_t)ctx->n_total + 63) / 64;   // 64-bit cells of dm_scratch, read as 32-bit words
    if (ctx->dm_scratch.ensure(cordon_words) != hipSuccess) {
      (void)hipGetLastError();
      raise(PE_ENOMEM, "cordon bitmap: device allocation failed");
    }
    uint32_t* const cordon = (uint32_t*)ctx->dm_scratch.p;
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    const pe::DrainMoveIn min{runs.in(d), pairs.in(d),      words.in(d) + L0 + ND, slots.in(d),
                              run_of.in(d), run_pair.in(d), cordon};
    const pe::DrainOut out{fits.in(o), moved.in(o), fail.in(o), store ? target.in(o) : nullptr};
    hipchk(hipMemsetAsync(cordon, 0, cordon_words * sizeof(int64_t), ctx->stream), "clear the cordon bitmap");
    if (store) hipchk(hipMemsetAsync(out.target, 0xFF, target.bytes(), ctx->stream), "clear targets");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, words.in(d), L0, A, segs);
    hipchk(pe::launch_drain_cordon(ctx->stream, pairs.in(d), C, cordon), "launch drain_cordon");
    hipchk(pe::launch_drain_move(ctx->stream, min, (int)A, segs, ctx->res.p, ctx->stride, (uint32_t)ctx->begin, dry, out,
                                 row.in(o), ctx->dm_log.p),
           "launch drain_move");
    if (store || !dry)
      hipchk(pe::launch_drain_move_sweep(ctx->stream, min, E, out.fits, row.in(o), out.target, ctx->res.p, ctx->stride,
                                         (uint32_t)ctx->begin, dry),
             "launch drain_move_sweep");
    ev.end();
    const uint8_t* const a = block_read_back(ctx, ans, "drain-move", "sync drain_move_domains");
    block_part_to(out_fits, fits, a);
    block_part_to(out_moved, moved, a);
    block_part_to(out_fail_slot, fail, a);
    block_part_to(out_target, target, a);
    if (!dry) {
      // the takes: candidate c is job c, its runs are its groups, placed where it fits; the counters stay
      std::vector<int32_t> status((size_t)C);
      for (int64_t c = 0; c < C; ++c) status[(size_t)c] = fits.in(a)[c] ? PE_JOB_PLACED : PE_JOB_UNSCHEDULABLE;
      const pe_stats kept = ctx->stats;
      mirror_follow(ctx, "drain_move_kernel", C, plan.run_start.data(), run_req.data(), pod_off.data(), row.in(a),
                    status.data());
      ctx->stats = kept;
      // the give-back: the mirror's release of exactly the slots that moved
      for (int64_t c = 0; c < C; ++c) {
        if (!fits.in(a)[c]) continue;
        pe::NodeState& m = ctx->m_nodes[(size_t)cand_node[c]];
        for (int32_t r = plan.run_start[(size_t)c]; r < plan.run_start[(size_t)c + 1]; ++r)
          for (int dd = 0; dd < pe::D; ++dd) m.res[dd] += plan.runs[(size_t)r].count * run_req[(size_t)(r * pe::D + dd)];
      }
    }
    ev.report_as("A=" + std::to_string(A) + " E=" + std::to_string(E));
    return PE_OK;
  });
}

}  // extern "C"
