// libplacement: the exact what-if of a whole gang per domain (pe_gang_fit_domains).  The host validates the batch,
// the hierarchy and the pair list and builds the plan (pe_fit_plan.h); the groups, the pair and unit tables and the
// plan's words cross in one pinned block and one copy; pe_place.hip's member kernels gather every active domain's
// nodes into a compact segment and the kernels of pe_fit.hip judge every pair on a private copy of its segment,
// one workgroup per unit of at most FIT_UNIT_PAIRS pairs; the answers the caller asked for come back in one copy.
// Read-only: the device residuals, the host mirror, the staged fit-mask state and the stats are not touched.  The
// host path and the buffers are the domain calls' (pe_domain_call.h, pe_ctx.h dm_*): nothing of the hierarchy, the
// batch or the pairs is kept between calls.
#include "pe_domain_call.h"

extern "C" {

int pe_gang_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                        const int64_t* group_req, const uint32_t* group_need, int64_t n_pairs, const int32_t* pair_job,
                        const int32_t* pair_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                        const int32_t* parent, uint8_t* out_fits, int32_t* out_fail_group, int64_t* out_pods,
                        int32_t* out_first) {
  return guarded(ctx, [&]() -> int {
    domain_entry_checks(ctx, "pe_gang_fit_domains", n_jobs);
    const int64_t G = n_jobs > 0 ? check_gang_groups(n_jobs, job_group_off, group_count, group_req) : 0;
    pe::FitPlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::FitPlanError err =
        pe::fit_plan_build(plan, n_jobs, n_pairs, pair_job, pair_domain, level, n_levels, level_size, parent, &te, &bad);
    if (err != pe::FIT_OK) raise_fit_plan(err, te, bad);
    const int64_t J = n_jobs, P = n_pairs, A = plan.n_active(), U = plan.n_units();
    if (P == 0) {   // no pair: nothing fits anywhere, and nothing runs
      if (out_first) std::fill(out_first, out_first + J, -1);
      return PE_OK;
    }
    const int64_t L0 = plan.n_leaf, ND = plan.n_dom;
    // ---- one pinned block in: the groups, the pairs in plan order, the units, then the plan's words
    pe::BlockLayout in;
    const auto groups = in.add<pe::PlaceGroup>(G);
    const auto pairs = in.add<pe::FitPair>(P);
    const auto units = in.add<pe::FitUnit>(U);
    const auto words = in.add<int32_t>(L0 + ND);
    uint8_t* const h = block_in_host(ctx, in, "gang-fit");
    fill_place_groups(groups.in(h), G, group_req, group_need, group_count, nullptr);
    pe::FitPair* const h_pairs = pairs.in(h);
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = plan.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::FitPair{p, j, job_group_off[j], job_group_off[j + 1]};
    }
    std::memcpy(units.in(h), plan.units.data(), units.bytes());
    pack_domain_words(words.in(h), plan.leaf_dom, plan.act_of);
    const uint8_t* const d = block_in_device(ctx, in, "gang-fit");
    // ---- the call's device buffers; the answers: first [J], then fits, fail_group and pods [P], 16-B aligned
    pe::BlockLayout ans;
    const auto first = ans.add<uint32_t>(J, 16, out_first != nullptr);
    const auto fits = ans.add<uint8_t>(P, 16, out_fits != nullptr);
    const auto fail = ans.add<int32_t>(P, 16, out_fail_group != nullptr);
    const auto pods = ans.add<int64_t>(P, 16, out_pods != nullptr);
    uint8_t* const o = block_out_device(ctx, ans, "gang-fit");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::FitOut out{first.in(o), fits.in(o), fail.in(o), pods.in(o)};
    hipchk(hipMemsetAsync(out.first, 0xFF, first.bytes(), ctx->stream), "clear first fits");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, words.in(d), L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_fit(ctx->stream, groups.in(d), pairs.in(d), units.in(d), blocks, large.recs, large.scratch, segs,
                            out),
             what);
    };
    launch_units_then_large(
        ctx, segs, A, plan, [&]() { launch(U, {}, "launch fit_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch fit_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const uint8_t* const a = block_read_back(ctx, ans, "gang-fit", "sync gang_fit_domains");
    block_part_to(out_first, first, a);   // ~0 reads as -1: no pair fits
    block_part_to(out_fits, fits, a);
    block_part_to(out_fail_group, fail, a);
    block_part_to(out_pods, pods, a);
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U));
    return PE_OK;
  });
}

}  // extern "C"
