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
    const size_t pairs_at = (size_t)G * sizeof(pe::PlaceGroup);
    const size_t units_at = pairs_at + (size_t)P * sizeof(pe::FitPair);
    const size_t words_at = units_at + (size_t)U * sizeof(pe::FitUnit);
    const size_t in_bytes = words_at + (size_t)(L0 + ND) * sizeof(int32_t);
    hipchk(ctx->dm_hin.ensure(in_bytes), "alloc pinned gang-fit inputs");
    hipchk(ctx->dm_in.ensure(in_bytes), "alloc gang-fit inputs");
    fill_place_groups((pe::PlaceGroup*)ctx->dm_hin.p, G, group_req, group_need, group_count, nullptr);
    pe::FitPair* const h_pairs = (pe::FitPair*)(ctx->dm_hin.p + pairs_at);
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = plan.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::FitPair{p, j, job_group_off[j], job_group_off[j + 1]};
    }
    std::memcpy(ctx->dm_hin.p + units_at, plan.units.data(), (size_t)U * sizeof(pe::FitUnit));
    pack_domain_words((int32_t*)(ctx->dm_hin.p + words_at), plan.leaf_dom, plan.act_of);
    hipchk(hipMemcpyAsync(ctx->dm_in.p, ctx->dm_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D gang-fit inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->dm_in.p;
    const pe::FitPair* const d_pairs = (const pe::FitPair*)(ctx->dm_in.p + pairs_at);
    const pe::FitUnit* const d_units = (const pe::FitUnit*)(ctx->dm_in.p + units_at);
    const int32_t* const d_words = (const int32_t*)(ctx->dm_in.p + words_at);
    // ---- the call's device buffers; the answers: first [J], then fits, fail_group and pods [P], 16-B aligned
    const size_t fits_at = r16((size_t)J * sizeof(int32_t));
    const size_t fail_at = fits_at + r16((size_t)P);
    const size_t pods_at = fail_at + r16((size_t)P * sizeof(int32_t));
    const size_t out_bytes = pods_at + (size_t)P * sizeof(int64_t);
    hipchk(ctx->dm_out.ensure(out_bytes), "alloc gang-fit outputs");
    const pe::PlaceSegs segs = domain_segments(ctx, A);
    pe::FitOut out{(uint32_t*)ctx->dm_out.p, ctx->dm_out.p + fits_at, (int32_t*)(ctx->dm_out.p + fail_at),
                   (int64_t*)(ctx->dm_out.p + pods_at)};
    hipchk(hipMemsetAsync(out.first, 0xFF, (size_t)J * sizeof(int32_t), ctx->stream), "clear first fits");
    CapEvents ev(ctx);
    ev.begin();
    launch_domain_members(ctx, d_words, L0, A, segs);
    const auto launch = [&](int64_t blocks, const LargeSegs& large, const char* what) {
      hipchk(pe::launch_fit(ctx->stream, d_groups, d_pairs, d_units, blocks, large.recs, large.scratch, segs, out), what);
    };
    launch_units_then_large(
        ctx, segs, A, plan, [&]() { launch(U, {}, "launch fit_domains (LDS)"); },
        [&](const LargeSegs& large) { launch(large.n, large, "launch fit_domains (global)"); });
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const bool tables = out_fits || out_fail_group || out_pods;
    const size_t lo = out_first ? 0 : out_fits ? fits_at : out_fail_group ? fail_at : pods_at;
    const size_t hi = out_pods         ? out_bytes
                      : out_fail_group ? fail_at + (size_t)P * sizeof(int32_t)
                      : out_fits       ? fits_at + (size_t)P
                                       : (size_t)J * sizeof(int32_t);
    if (out_first || tables) {
      hipchk(ctx->dm_hout.ensure(hi), "alloc pinned gang-fit outputs");
      hipchk(hipMemcpyAsync(ctx->dm_hout.p + lo, ctx->dm_out.p + lo, hi - lo, hipMemcpyDeviceToHost, ctx->stream),
             "D2H gang-fit answers");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync gang_fit_domains");
    const uint8_t* const h = ctx->dm_hout.p;
    if (out_first) std::memcpy(out_first, h, (size_t)J * sizeof(int32_t));   // ~0 reads as -1: no pair fits
    if (out_fits) std::memcpy(out_fits, h + fits_at, (size_t)P);
    if (out_fail_group) std::memcpy(out_fail_group, h + fail_at, (size_t)P * sizeof(int32_t));
    if (out_pods) std::memcpy(out_pods, h + pods_at, (size_t)P * sizeof(int64_t));
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U));
    return PE_OK;
  });
}

}  // extern "C"
