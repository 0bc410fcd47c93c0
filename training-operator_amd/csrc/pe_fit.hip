// Exact what-if of a whole gang per domain (pe_gang_fit_domains): would pe_place_greedy_domains, given this one
// job in this domain against the current residuals, place it?  Every (job, domain) pair is judged alone, so
// unlike the placement itself the work is fully parallel: the plan (pe_fit_plan.h) cuts each active domain's
// pairs into WORK UNITS of at most FIT_UNIT_PAIRS pairs, and one workgroup per unit judges its pairs one after
// the other.
//
// Member lists: pe_place.hip's launch_place_members -- every active domain's nodes gathered into a compact
// segment of global id, labels and four residual rows.  This call only reads them.
//
// fit_domains_kernel: the what-if frame (pe_what_if.h: units, working state in LDS or in the global scratch, two
// instances, the fresh copy per pair) around this file's own lines: per pair they run the job's groups
// through the placement's walk (pe_place_step.h: the same node_key, take and argmin, one barrier per decision,
// take-many, an island group as one decision), which stops at the first pod that finds no node, and sum the
// pods placed.  There is no log, no pod store and no rollback: the next pair's copy discards the state, at about
// the cost of one decision's scan.  Thread i mod PL_THREADS is the only one that touches place i -- in the copy
// as in the decisions -- so the copy needs no barrier.  Thread 0 stores the pair's three answers and lowers
// first[job] to the pair's index if it fits (an unsigned minimum over cells the host set to ~0, which read as
// -1 where no pair fits).
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_what_if.h"

namespace pe {

namespace {

// what_if_units' body: per pair a fresh copy, the job's groups through the walk, the three answers.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void fit_domains_kernel(
    const PlaceGroup* __restrict__ groups, const FitPair* __restrict__ pairs, const FitUnit* __restrict__ units,
    const FitLarge* __restrict__ large, int64_t* __restrict__ scratch, const int32_t* __restrict__ seg_off,
    const uint32_t* __restrict__ seg_gid, const uint32_t* __restrict__ seg_lab, const int64_t* __restrict__ seg_res,
    int64_t ss, FitOut out) {
  what_if_units<IN_LDS>(
      units, large, scratch, seg_off, seg_gid, seg_lab, seg_res, ss,
      [&](int64_t* w0, auto ws, const int64_t* src, int64_t rs, const uint32_t* gid, const uint32_t* lab, int, int n,
          PlaceMin& mn, int& par, int p0, int p1) {
        for (int pi = p0; pi < p1; ++pi) {
          const FitPair pr = pairs[pi];
          what_if_copy(w0, ws, src, rs, n);   // the pair is judged alone
          int64_t placed = 0;   // pods the rule has placed so far
          uint32_t left;
          const int g = place_groups(w0, ws, gid, lab, n, mn, par, groups, pr.g0, pr.g1, left,
                                     [&](int, const PlaceGroup&, const PlaceChoice& c, uint32_t) { placed += c.t; });
          const int fail = g < pr.g1 ? g - pr.g0 : -1;   // the first group, from the job's first, not placed in full
          if (threadIdx.x == 0) {   // pr.pair < P, pr.job < J: the plan validated the list
            out.fits[pr.pair] = fail < 0;
            out.fail_group[pr.pair] = fail;
            out.pods[pr.pair] = placed;
            if (fail < 0) atomicMin(&out.first[pr.job], (uint32_t)pr.pair);
          }
        }
      });
}

}  // namespace

hipError_t launch_fit(hipStream_t s, const PlaceGroup* groups, const FitPair* pairs, const FitUnit* units, int64_t blocks,
                      const FitLarge* large, int64_t* scratch, const PlaceSegs& segs, const FitOut& out) {
  if (blocks <= 0) return hipSuccess;
  if (blocks > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(large ? fit_domains_kernel<false> : fit_domains_kernel<true>, dim3((unsigned)blocks), dim3(PL_THREADS),
                     0, s, groups, pairs, units, large, scratch, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid,
                     (const uint32_t*)segs.lab, (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
