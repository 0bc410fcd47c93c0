// libplacement: giving back and re-taking placed gangs (pe_release_gangs, pe_assume_gangs).  The host validates the
// gangs and builds the plan against its mirror (pe_ledger_plan.h): the new absolute residuals of every node the
// gangs touch, or the node at which the call's bound is crossed -- then nothing has changed.  The records of this
// shard's touched nodes cross in one pinned block and one copy and pe_ledger.hip scatters them into the device
// residuals; the mirror, which holds the GLOBAL inventory, takes every touched node once the device part has
// succeeded.  No exchange: every rank of a sharded context makes the same call and decides alike on its own mirror.
// The reset snapshot, labels, islands, the staged fit batch and the stats are not touched.  Own buffers (pe_ctx.h
// ld_*): nothing of the gangs is kept between calls.
#include <chrono>

#include "pe_ctx.h"

namespace {

[[noreturn]] void raise_gangs(pe::GangSlotsError e, int64_t bad) {
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

int ledger_call(pe_ctx* ctx, pe::LedgerOp op, int64_t n_gangs, const int32_t* gang_group_off, const int32_t* group_count,
                const int64_t* group_req, const int32_t* pod_node, int64_t* out_pods) {
  return guarded(ctx, [&]() -> int {
    const char* const name = op == pe::LEDGER_RELEASE ? "pe_release_gangs" : "pe_assume_gangs";
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (n_gangs < 0) raise(PE_EINVAL, "n_gangs < 0");
    CapEvents ev(ctx);
    const auto t0 = std::chrono::steady_clock::now();
    pe::GangSlotsError ge = pe::GANGS_OK;
    int64_t bad = -1;
    const pe::LedgerPlanError err = pe::ledger_plan_build(
        ctx->ld_plan, op, ctx->n_total, n_gangs, gang_group_off, group_count, group_req, pod_node,
        [ctx](int32_t n) { return ctx->m_nodes[(size_t)n].res; }, [ctx](int32_t n) { return ctx->m_nodes0[(size_t)n].res; },
        &ge, &bad);
    if (err == pe::LEDGER_BAD_GANGS) raise_gangs(ge, bad);
    if (err == pe::LEDGER_OVER)
      raise(PE_EINVAL, std::string(name) + ": more is given back than was taken (the residual would exceed the reset "
                                           "snapshot) at node " + std::to_string(bad));
    if (err == pe::LEDGER_UNDER)
      raise(PE_EINVAL, std::string(name) + ": the pods do not fit (the residual would fall below 0) at node " +
                           std::to_string(bad));
    const pe::LedgerPlan& plan = ctx->ld_plan;
    // ---- one pinned block in: this shard's touched nodes by their local index
    int64_t T = 0;
    if (!plan.touched.empty() && ctx->Ns > 0) {
      hipchk(ctx->ld_hin.ensure(std::min<size_t>(plan.touched.size(), (size_t)ctx->Ns)), "alloc pinned ledger records");
      for (const pe::LedgerUpd& u : plan.touched) {
        if (u.node < ctx->begin || u.node >= ctx->end) continue;
        pe::LedgerRec& r = ctx->ld_hin.p[T++];
        r.local = u.node - ctx->begin;
        for (int d = 0; d < pe::D; ++d) r.res[d] = u.res[d];
      }
    }
    const double plan_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (T > 0) {
      hipchk(ctx->ld_in.ensure((size_t)T), "alloc ledger records");
      hipchk(hipMemcpyAsync(ctx->ld_in.p, ctx->ld_hin.p, (size_t)T * sizeof(pe::LedgerRec), hipMemcpyHostToDevice,
                            ctx->stream),
             "H2D ledger records");
      ev.begin();
      hipchk(pe::launch_ledger_scatter(ctx->stream, ctx->res.p, ctx->stride, ctx->ld_in.p, T), "launch ledger_scatter");
      ev.end();
      hipchk(hipStreamSynchronize(ctx->stream), name);   // the pinned block is the next call's
    }
    // ---- the device holds the new values: the mirror follows, every rank the whole of it
    for (const pe::LedgerUpd& u : plan.touched) {
      pe::NodeState& m = ctx->m_nodes[(size_t)u.node];
      for (int d = 0; d < pe::D; ++d) m.res[d] = u.res[d];
    }
    if (out_pods) *out_pods = plan.pods;
    ev.report_as("T=" + std::to_string(T) + " steps=" + std::to_string(plan.steps) +
                 " plan_us=" + std::to_string(plan_us));
    return PE_OK;
  });
}

}  // namespace

extern "C" {

int pe_release_gangs(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off, const int32_t* group_count,
                     const int64_t* group_req, const int32_t* pod_node, int64_t* out_pods) {
  return ledger_call(ctx, pe::LEDGER_RELEASE, n_gangs, gang_group_off, group_count, group_req, pod_node, out_pods);
}

int pe_assume_gangs(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off, const int32_t* group_count,
                    const int64_t* group_req, const int32_t* pod_node, int64_t* out_pods) {
  return ledger_call(ctx, pe::LEDGER_ASSUME, n_gangs, gang_group_off, group_count, group_req, pod_node, out_pods);
}

}  // extern "C"
