// libplacement: why a pod shape fits no node (pe_fit_explain).  The host validates the batch and, where the jobs
// name domains, the hierarchy (pe_explain_plan.h), reduces the batch to its distinct (request, need, domain)
// records in first-seen order and walks the parent map to the leaf -> level-domain table; the records and the
// table cross in one pinned block and one copy; fit_explain_kernel (pe_explain.hip) fills the [S][32] counts and
// the [S][4] near values for one chunk of records per launch (the tables of a launch stay within 64 MiB); they
// come back with one copy and are scattered to the jobs here.  Read-only: the device residuals, the host mirror,
// the reset snapshot, the staged fit-mask state and the stats are not touched.  Own buffers (pe_ctx.h ex_*; the
// events are the capacity calls'): nothing of the hierarchy or the batch is kept between calls.
#include "pe_ctx.h"

static_assert(pe::EX_BINS == PE_EXPLAIN_BINS && pe::EX_ANY == PE_EXPLAIN_ANY && pe::EX_DIMS == pe::D,
              "pe_explain_plan.h");
static_assert(PE_EXPLAIN_LABELS == pe::EX_DIMS, "the label test is the signature bit behind the dimensions");

extern "C" {

int pe_fit_explain(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* job_domain,
                   int32_t level, int32_t n_levels, const int32_t* level_size, const int32_t* parent, int64_t* out_hist,
                   uint64_t* out_near) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (n_jobs == 0) return PE_OK;
    if (n_jobs > (int64_t)INT32_MAX) raise(PE_EINVAL, "n_jobs above 2^31 - 1");
    pe::TreePlanError te = pe::TREE_OK;
    int64_t bad = -1;
    switch (pe::explain_validate(n_jobs, req, job_domain, level, n_levels, level_size, parent, &te, &bad)) {
      case pe::EX_OK: break;
      case pe::EX_NO_REQ: raise(PE_EINVAL, "req is NULL");
      case pe::EX_BAD_REQ: raise(PE_EINVAL, "req: negative request at index " + std::to_string(bad));
      case pe::EX_BAD_TREE: raise_tree(te, bad);
      case pe::EX_BAD_LEVEL: raise(PE_EINVAL, "level outside [0, n_levels)");
      case pe::EX_BAD_DOMAIN:
        raise(PE_EINVAL, "job_domain: value outside [PE_EXPLAIN_ANY, level_size[level]) at index " + std::to_string(bad));
    }
    if (!out_hist && !out_near) return PE_OK;
    constexpr int64_t B = pe::EX_BINS, Dn = pe::EX_DIMS;
    if (ctx->Ns == 0) {   // an empty shard has no live node
      if (out_hist) std::memset(out_hist, 0, (size_t)(n_jobs * B) * sizeof(int64_t));
      if (out_near) std::memset(out_near, 0, (size_t)(n_jobs * Dn) * sizeof(uint64_t));
      return PE_OK;
    }
    const int64_t S = pe::explain_dedupe(n_jobs, req, need, job_domain, ctx->ex_tab, ctx->ex_of, ctx->ex_uniq);
    const bool domains = job_domain != nullptr;
    int64_t n_leaf = 0;
    if (domains) {
      pe::explain_leaf_dom(level, level_size, parent, ctx->ex_leaf);
      n_leaf = (int64_t)ctx->ex_leaf.size();
    }
    CapEvents ev(ctx);
    // one block and one copy in: the records (64 B each), then the leaf -> level-domain table
    const size_t rec_bytes = (size_t)S * sizeof(pe::ExplainRec), in_bytes = rec_bytes + (size_t)n_leaf * sizeof(int32_t);
    hipchk(ctx->ex_hin.ensure(in_bytes), "alloc pinned explain records");
    hipchk(ctx->ex_in.ensure(in_bytes), "alloc explain records");
    std::memcpy((void*)ctx->ex_hin.p, ctx->ex_uniq.data(), rec_bytes);
    if (n_leaf) std::memcpy((void*)(ctx->ex_hin.p + rec_bytes), ctx->ex_leaf.data(), (size_t)n_leaf * sizeof(int32_t));
    hipchk(hipMemcpyAsync(ctx->ex_in.p, ctx->ex_hin.p, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D explain records");
    const pe::ExplainRec* const d_recs = (const pe::ExplainRec*)ctx->ex_in.p;
    const int32_t* const d_leaf = domains ? (const int32_t*)(ctx->ex_in.p + rec_bytes) : nullptr;
    // a launch's tables: the chunk's counts [sc][32], then (when asked for) its near values [sc][4]
    const int64_t W = out_near ? pe::EX_OUT_WORDS : B;
    const int64_t chunk = pe::explain_chunk(S, pe::EX_BUDGET_BYTES);
    hipchk(ctx->ex_out.ensure((size_t)(chunk * W)), "alloc explain tables");
    hipchk(ctx->ex_hout.ensure((size_t)(S * W)), "alloc pinned explain tables");
    ev.begin();
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int64_t sc = std::min(chunk, S - s0);
      uint64_t* const d_hist = ctx->ex_out.p;
      uint64_t* const d_near = out_near ? d_hist + sc * B : nullptr;
      hipchk(hipMemsetAsync(d_hist, 0, (size_t)(sc * B) * sizeof(uint64_t), ctx->stream), "zero explain counts");
      if (d_near)
        hipchk(hipMemsetAsync(d_near, 0xFF, (size_t)(sc * Dn) * sizeof(uint64_t), ctx->stream), "preset near values");
      hipchk(pe::launch_fit_explain(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns, d_leaf,
                                    (int)n_leaf, domains, d_recs + s0, sc, d_hist, d_near),
             "launch fit_explain");
      if (s0 + sc == S) ev.end();
      hipchk(hipMemcpyAsync(ctx->ex_hout.p + s0 * W, d_hist, (size_t)(sc * W) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H explain tables");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync fit_explain");
    const auto& of = ctx->ex_of;
    for (int64_t j = 0; j < n_jobs; ++j) {   // record of[j] lies in launch s0 = of[j] / chunk * chunk, of sc records
      const int64_t u = of[(size_t)j], s0 = u / chunk * chunk, sc = std::min(chunk, S - s0);
      const uint64_t* const base = ctx->ex_hout.p + s0 * W;
      if (out_hist) std::memcpy(out_hist + j * B, base + (u - s0) * B, (size_t)B * sizeof(int64_t));   // counts <= Ns
      if (out_near) {
        const uint64_t* v = base + sc * B + (u - s0) * Dn;
        for (int d = 0; d < Dn; ++d) out_near[j * Dn + d] = v[d] == ~uint64_t(0) ? 0 : v[d];
      }
    }
    ev.report(S);
    return PE_OK;
  });
}

}  // extern "C"
