// Exact what-if of a whole gang per domain (pe_gang_fit_domains): would pe_place_greedy_domains, given this one
// job in this domain against the current residuals, place it?  Every (job, domain) pair is judged alone, so
// unlike the placement itself the work is fully parallel: the plan (pe_fit_plan.h) cuts each active domain's
// pairs into WORK UNITS of at most FIT_UNIT_PAIRS pairs, and one workgroup per unit judges its pairs one after
// the other.
//
// Member lists: pe_place.hip's launch_place_members -- every active domain's nodes gathered into a compact
// segment of global id, labels and four residuals.  This call only reads them.
//
// fit_domains_kernel: per pair the workgroup copies the segment's four residual rows into its working state,
// runs the job's groups through the placement's decision (pe_place_step.h: the same node_key, take and argmin,
// one barrier per decision, take-many, an island group as one decision) and stops at the first pod that finds
// no node.  There is no log, no pod store and no rollback: the next pair's copy discards the state, at about
// the cost of one decision's scan.  Thread i mod PL_THREADS is the only one that touches place i -- in the copy
// as in the decisions -- so the copy needs no barrier.  Thread 0 stores the pair's three answers and lowers
// first[job] to the pair's index if it fits (an unsigned minimum over cells the host set to ~0, which read as
// -1 where no pair fits).  The working state lives in LDS for segments of at most PL_LDS_NODES nodes, laid out
// as the placement's PlaceShared with the ids and labels staged once per unit; a larger segment's units work on
// private rows of a global scratch array whose size the host bounds (pe_fit_plan.h fit_scratch_layout), a few
// workgroups per domain striding over its units.  Two instances, as in pe_place.hip.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_fit_plan.h"
#include "pe_kernels.h"
#include "pe_place_step.h"

namespace pe {

namespace {

// The pairs at places [p0, p1) of the plan's list, all of one segment: n nodes with ids gid[i], labels lab[i]
// and residuals src[d * ss + i] (read), judged on the working state w0[d * ws + i] (written).
template <class Stride>
__device__ __forceinline__ void fit_pairs(int64_t* w0, Stride ws, const int64_t* __restrict__ src, int64_t ss,
                                          const uint32_t* gid, const uint32_t* lab, int n, PlaceMin& mn, int& par,
                                          const PlaceGroup* __restrict__ groups, const FitPair* __restrict__ pairs,
                                          int p0, int p1, const FitOut& out) {
  const int tid = threadIdx.x;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  for (int pi = p0; pi < p1; ++pi) {
    const FitPair pr = pairs[pi];
    for (int i = tid; i < n; i += PL_THREADS) {   // a fresh copy: the pair is judged alone
      w0[i] = src[i];
      w1[i] = src[ss + i];
      w2[i] = src[2 * ss + i];
      w3[i] = src[3 * ss + i];
    }
    int64_t placed = 0;   // pods the rule has placed so far
    int fail = -1;        // the first group, counted from the job's first, that was not placed in full
    for (int g = pr.g0; g < pr.g1 && fail < 0; ++g) {
      const PlaceGroup gr = groups[g];
      if (gr.count <= 0) continue;
      const bool unit = (gr.need & NEED_ISLAND) != 0;   // an island group: one decision for count x request
      int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
      if (unit && !island_request(gr, s0, s1, s2, s3)) {   // fits nowhere
        fail = g - pr.g0;
        break;
      }
      uint32_t left = (uint32_t)gr.count;
      while (left > 0) {
        const PlaceChoice c = place_decide(w0, w1, w2, w3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, left, mn, par);
        if (c.none()) {   // no node of the domain fits
          fail = g - pr.g0;
          break;
        }
        place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3);
        placed += c.t;
        left -= c.t;
      }
    }
    if (tid == 0) {   // pr.pair < P, pr.job < J: the plan validated the list
      out.fits[pr.pair] = fail < 0;
      out.fail_group[pr.pair] = fail;
      out.pods[pr.pair] = placed;
      if (fail < 0) atomicMin(&out.first[pr.job], (uint32_t)pr.pair);
    }
  }
}

// IN_LDS: one workgroup per unit, for the units whose segment has at most PL_LDS_NODES nodes (a workgroup whose
// segment is larger leaves at once); the other instance has one workgroup per FitLarge record.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void fit_domains_kernel(
    const PlaceGroup* __restrict__ groups, const FitPair* __restrict__ pairs, const FitUnit* __restrict__ units,
    const FitLarge* __restrict__ large, int64_t* __restrict__ scratch, const int32_t* __restrict__ seg_off,
    const uint32_t* __restrict__ seg_gid, const uint32_t* __restrict__ seg_lab, const int64_t* __restrict__ seg_res,
    int64_t ss, FitOut out) {
  __shared__ PlaceMin mn;
  const int tid = threadIdx.x;
  int par = 0;
  if constexpr (IN_LDS) {
    const FitUnit u = units[blockIdx.x];
    const int b = seg_off[u.act], n = seg_off[u.act + 1] - b;
    if (n > PL_LDS_NODES) return;
    __shared__ PlaceShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
      sh.gid[i] = seg_gid[b + i];
      sh.lab[i] = seg_lab[b + i];
    }
    fit_pairs(sh.r[0], std::integral_constant<int, PL_LDS_NODES>(), seg_res + b, ss, sh.gid, sh.lab, n, mn, par, groups,
              pairs, u.p0, u.p1, out);
  } else {
    const FitLarge w = large[blockIdx.x];
    const int b = seg_off[w.act], n = seg_off[w.act + 1] - b;
    for (int u = w.u0 + w.s; u < w.u1; u += w.k)   // the copy holds 4 n cells from w.at: the host laid it out for this n
      fit_pairs(scratch + w.at, (int64_t)n, seg_res + b, ss, seg_gid + b, seg_lab + b, n, mn, par, groups, pairs,
                units[u].p0, units[u].p1, out);
  }
}

}  // namespace

hipError_t launch_fit_units(hipStream_t s, const PlaceGroup* groups, const FitPair* pairs, const FitUnit* units, int64_t U,
                            const PlaceSegs& segs, const FitOut& out) {
  if (U <= 0) return hipSuccess;
  if (U > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_domains_kernel<true>, dim3((unsigned)U), dim3(PL_THREADS), 0, s, groups, pairs, units,
                     (const FitLarge*)nullptr, (int64_t*)nullptr, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid,
                     (const uint32_t*)segs.lab, (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

hipError_t launch_fit_large(hipStream_t s, const PlaceGroup* groups, const FitPair* pairs, const FitUnit* units,
                            const FitLarge* large, int64_t n_large, int64_t* scratch, const PlaceSegs& segs,
                            const FitOut& out) {
  if (n_large <= 0) return hipSuccess;
  if (n_large > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fit_domains_kernel<false>, dim3((unsigned)n_large), dim3(PL_THREADS), 0, s, groups, pairs, units, large,
                     scratch, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid, (const uint32_t*)segs.lab,
                     (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
