// libplacement: the exact what-if of a whole gang per domain (pe_gang_fit_domains).  The host validates the batch,
// the hierarchy and the pair list and builds the plan (pe_fit_plan.h); the groups, the pair and unit tables and the
// plan's words cross in one pinned block and one copy; pe_place.hip's member kernels gather every active domain's
// nodes into a compact segment and the kernels of pe_fit.hip judge every pair on a private copy of its segment,
// one workgroup per unit of at most FIT_UNIT_PAIRS pairs; the answers the caller asked for come back in one copy.
// Read-only: the device residuals, the host mirror, the staged fit-mask state and the stats are not touched.  Own
// buffers (pe_ctx.h ft_*): nothing of the hierarchy, the batch or the pairs is kept between calls.
#include "pe_ctx.h"
#include "pe_fit_plan.h"

namespace {

[[noreturn]] void raise_plan(pe::FitPlanError e, pe::TreePlanError te, int64_t bad) {
  switch (e) {
    case pe::FIT_BAD_LEVEL: raise(PE_EINVAL, "level outside [0, n_levels)");
    case pe::FIT_BAD_COUNT: raise(PE_EINVAL, "n_pairs outside [0, 2^31 - 1)");
    case pe::FIT_NO_PAIRS: raise(PE_EINVAL, "pair_job or pair_domain is NULL");
    case pe::FIT_BAD_JOB: raise(PE_EINVAL, "pair_job: value outside [0, n_jobs) at index " + std::to_string(bad));
    case pe::FIT_BAD_DOMAIN:
      raise(PE_EINVAL, "pair_domain: value outside [0, level_size[level]) at index " + std::to_string(bad));
    default: raise_tree(te, bad);
  }
}

size_t r16(size_t x) { return (x + 15) & ~size_t(15); }

}  // namespace

extern "C" {

int pe_gang_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                        const int64_t* group_req, const uint32_t* group_need, int64_t n_pairs, const int32_t* pair_job,
                        const int32_t* pair_domain, int32_t level, int32_t n_levels, const int32_t* level_size,
                        const int32_t* parent, uint8_t* out_fits, int32_t* out_fail_group, int64_t* out_pods,
                        int32_t* out_first) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (ctx->world > 1) raise(PE_EINVAL, "pe_gang_fit_domains on a sharded context: a domain may span shards");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    const int64_t G = n_jobs > 0 ? check_gang_groups(n_jobs, job_group_off, group_count, group_req) : 0;
    pe::FitPlan plan;
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    const pe::FitPlanError err =
        pe::fit_plan_build(plan, n_jobs, n_pairs, pair_job, pair_domain, level, n_levels, level_size, parent, &te, &bad);
    if (err != pe::FIT_OK) raise_plan(err, te, bad);
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
    hipchk(ctx->ft_hin.ensure(in_bytes), "alloc pinned gang-fit inputs");
    hipchk(ctx->ft_in.ensure(in_bytes), "alloc gang-fit inputs");
    pe::PlaceGroup* const h_groups = (pe::PlaceGroup*)ctx->ft_hin.p;
    for (int64_t g = 0; g < G; ++g) {
      pe::PlaceGroup& r = h_groups[g];
      std::memset(&r, 0, sizeof(r));
      for (int d = 0; d < pe::D; ++d) r.q[d] = group_req[g * pe::D + d];
      r.need = group_need ? group_need[g] : 0u;
      r.count = group_count[g];
    }
    pe::FitPair* const h_pairs = (pe::FitPair*)(ctx->ft_hin.p + pairs_at);
    for (int64_t i = 0; i < P; ++i) {
      const int32_t p = plan.pairs[(size_t)i], j = pair_job[p];
      h_pairs[i] = pe::FitPair{p, j, job_group_off[j], job_group_off[j + 1]};
    }
    std::memcpy(ctx->ft_hin.p + units_at, plan.units.data(), (size_t)U * sizeof(pe::FitUnit));
    int32_t* const h_words = (int32_t*)(ctx->ft_hin.p + words_at);
    std::memcpy(h_words, plan.leaf_dom.data(), (size_t)L0 * sizeof(int32_t));
    std::memcpy(h_words + L0, plan.act_of.data(), (size_t)ND * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->ft_in.p, ctx->ft_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D gang-fit inputs");
    const pe::PlaceGroup* const d_groups = (const pe::PlaceGroup*)ctx->ft_in.p;
    const pe::FitPair* const d_pairs = (const pe::FitPair*)(ctx->ft_in.p + pairs_at);
    const pe::FitUnit* const d_units = (const pe::FitUnit*)(ctx->ft_in.p + units_at);
    const int32_t* const d_words = (const int32_t*)(ctx->ft_in.p + words_at);
    // ---- the call's device buffers; the answers: first [J], then fits, fail_group and pods [P], 16-B aligned
    const int64_t st = std::max<int64_t>(ctx->stride, 1);
    const size_t fits_at = r16((size_t)J * sizeof(int32_t));
    const size_t fail_at = fits_at + r16((size_t)P);
    const size_t pods_at = fail_at + r16((size_t)P * sizeof(int32_t));
    const size_t out_bytes = pods_at + (size_t)P * sizeof(int64_t);
    hipchk(ctx->ft_out.ensure(out_bytes), "alloc gang-fit outputs");
    hipchk(ctx->ft_dom.ensure((size_t)(3 * A + 1)), "alloc domain lists");
    hipchk(ctx->ft_seg.ensure((size_t)(pe::D * st)), "alloc domain segments");
    hipchk(ctx->ft_segw.ensure((size_t)(2 * st)), "alloc domain segments");
    pe::PlaceSegs segs{};
    segs.cnt = ctx->ft_dom.p;
    segs.seg_off = ctx->ft_dom.p + A;
    segs.cursor = ctx->ft_dom.p + 2 * A + 1;
    segs.gid = ctx->ft_segw.p;
    segs.lab = ctx->ft_segw.p + st;
    segs.res = ctx->ft_seg.p;
    segs.seg_stride = st;
    pe::FitOut out{(uint32_t*)ctx->ft_out.p, ctx->ft_out.p + fits_at, (int32_t*)(ctx->ft_out.p + fail_at),
                   (int64_t*)(ctx->ft_out.p + pods_at)};
    hipchk(hipMemsetAsync(segs.cnt, 0, (size_t)A * sizeof(int32_t), ctx->stream), "zero domain counts");
    hipchk(hipMemsetAsync(out.first, 0xFF, (size_t)J * sizeof(int32_t), ctx->stream), "clear first fits");
    CapEvents ev(ctx);
    ev.begin();
    hipchk(pe::launch_place_members(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                    (uint64_t)ctx->begin, d_words, (int)L0, d_words + L0, (int)A, segs),
           "launch place_members");
    // a segment above PL_LDS_NODES nodes needs the shard to have that many: only then the bounds come back, while
    // the units of the smaller segments already run
    const bool may_be_large = ctx->Ns > pe::PL_LDS_NODES;
    if (may_be_large) {
      hipchk(ctx->ft_hoff.ensure((size_t)(A + 1)), "alloc pinned segment bounds");
      hipchk(hipMemcpyAsync(ctx->ft_hoff.p, segs.seg_off, (size_t)(A + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H segment bounds");
      if (!ctx->ft_ev) hipchk(hipEventCreateWithFlags(&ctx->ft_ev, hipEventDisableTiming), "event create");
      hipchk(hipEventRecord(ctx->ft_ev, ctx->stream), "event record");
    }
    hipchk(pe::launch_fit_units(ctx->stream, d_groups, d_pairs, d_units, U, segs, out), "launch fit_domains (LDS)");
    if (may_be_large) {
      hipchk(hipEventSynchronize(ctx->ft_ev), "wait for the segment bounds");
      std::vector<pe::FitLarge> large;
      const int64_t nodes = pe::fit_scratch_layout(plan, ctx->ft_hoff.p, ctx->Ns, pe::PL_LDS_NODES, large);
      if (!large.empty()) {
        const size_t bytes = large.size() * sizeof(pe::FitLarge);
        hipchk(ctx->ft_hlarge.ensure(bytes), "alloc pinned large-segment records");
        hipchk(ctx->ft_large.ensure(bytes), "alloc large-segment records");
        if (ctx->ft_scratch.ensure((size_t)(pe::D * nodes)) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipStreamSynchronize(ctx->stream);   // the units already queued touch the call's own buffers only
          raise(PE_ENOMEM, "working copies of the large segments: device allocation failed");
        }
        std::memcpy(ctx->ft_hlarge.p, large.data(), bytes);
        hipchk(hipMemcpyAsync(ctx->ft_large.p, ctx->ft_hlarge.p, bytes, hipMemcpyHostToDevice, ctx->stream),
               "H2D large-segment records");
        hipchk(pe::launch_fit_large(ctx->stream, d_groups, d_pairs, d_units, (const pe::FitLarge*)ctx->ft_large.p,
                                    (int64_t)large.size(), ctx->ft_scratch.p, segs, out),
               "launch fit_domains (global)");
      }
    }
    ev.end();
    // ---- one copy out: the span from the first to the last answer the caller asked for
    const bool tables = out_fits || out_fail_group || out_pods;
    const size_t lo = out_first ? 0 : out_fits ? fits_at : out_fail_group ? fail_at : pods_at;
    const size_t hi = out_pods         ? out_bytes
                      : out_fail_group ? fail_at + (size_t)P * sizeof(int32_t)
                      : out_fits       ? fits_at + (size_t)P
                                       : (size_t)J * sizeof(int32_t);
    if (out_first || tables) {
      hipchk(ctx->ft_hout.ensure(hi), "alloc pinned gang-fit outputs");
      hipchk(hipMemcpyAsync(ctx->ft_hout.p + lo, ctx->ft_out.p + lo, hi - lo, hipMemcpyDeviceToHost, ctx->stream),
             "D2H gang-fit answers");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync gang_fit_domains");
    const uint8_t* const h = ctx->ft_hout.p;
    if (out_first) std::memcpy(out_first, h, (size_t)J * sizeof(int32_t));   // ~0 reads as -1: no pair fits
    if (out_fits) std::memcpy(out_fits, h + fits_at, (size_t)P);
    if (out_fail_group) std::memcpy(out_fail_group, h + fail_at, (size_t)P * sizeof(int32_t));
    if (out_pods) std::memcpy(out_pods, h + pods_at, (size_t)P * sizeof(int64_t));
    ev.report_as("A=" + std::to_string(A) + " U=" + std::to_string(U));
    return PE_OK;
  });
}

}  // extern "C"
