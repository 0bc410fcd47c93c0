// The frame of the read-only what-if kernels (pe_fit.hip, pe_preempt.hip, pe_drain.hip, pe_scale.hip; device code
// only): each judges the pairs of its units on a private working copy of their segment's four residual rows, which a
// fresh copy per judgement discards.  what_if_units finds the workgroup's units and working state and hands them to the
// kernel's body, what_if_copy is the fresh copy; the groups' walk is pe_place_step.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pe_fit_plan.h"
#include "pe_kernels.h"
#include "pe_place_step.h"

namespace pe {

// IN_LDS: one workgroup per unit, for the units whose segment has at most PL_LDS_NODES nodes (a workgroup whose
// segment is larger leaves at once): the working state is a PlaceShared with the ids and labels staged once.  The
// other instance has one workgroup per FitLarge record, striding over the record's units on its private rows of
// the global scratch array whose size the host bounds (pe_fit_plan.h fit_scratch_layout).
// body(w0, ws, src, ss, gid, lab, b, n, mn, par, p0, p1) per unit: the pairs at places [p0, p1) of the plan's list,
// all of one segment -- n nodes at places [b, b + n) of the segments' arrays with ids gid[i], labels lab[i] and
// residuals src[d * ss + i] (read) -- to be judged on the working state w0[d * ws + i] (written).
// The pointers are the kernel's own __restrict__ parameters; said again here it cost preempt_domains_kernel<false>
// two VGPRs (profiles/domain_walk_refactor.txt).
template <bool IN_LDS, class Body>
__device__ __forceinline__ void what_if_units(const FitUnit* units, const FitLarge* large, int64_t* scratch,
                                              const int32_t* seg_off, const uint32_t* seg_gid, const uint32_t* seg_lab,
                                              const int64_t* seg_res, int64_t ss, Body&& body) {
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
    body(sh.r[0], std::integral_constant<int, PL_LDS_NODES>(), seg_res + b, ss, sh.gid, sh.lab, b, n, mn, par, u.p0, u.p1);
  } else {
    const FitLarge w = large[blockIdx.x];
    const int b = seg_off[w.act], n = seg_off[w.act + 1] - b;
    for (int u = w.u0 + w.s; u < w.u1; u += w.k)   // the copy holds 4 n cells from w.at: the host laid it out for this n
      body(scratch + w.at, (int64_t)n, seg_res + b, ss, seg_gid + b, seg_lab + b, b, n, mn, par, units[u].p0, units[u].p1);
  }
}

// A fresh copy of the segment's residuals into the working state, every thread its own places: no barrier.
// WITHOUT: the place whose id is `gone` reads NEVER in all four rows -- what a removed slot holds, so that no
// request, not even a zero one, fits it.  (Four rows through four pointers: written as a loop over d with
// w0[d * ws + i], the copy cost the global instances 11 VGPRs.)
template <bool WITHOUT = false, class Stride>
__device__ __forceinline__ void what_if_copy(int64_t* w0, Stride ws, const int64_t* __restrict__ src, int64_t ss, int n,
                                             const uint32_t* gid = nullptr, uint32_t gone = 0) {
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  for (int i = threadIdx.x; i < n; i += PL_THREADS) {
    bool out_of_it = false;
    if constexpr (WITHOUT) out_of_it = gid[i] == gone;
    w0[i] = out_of_it ? NEVER : src[i];
    w1[i] = out_of_it ? NEVER : src[ss + i];
    w2[i] = out_of_it ? NEVER : src[2 * ss + i];
    w3[i] = out_of_it ? NEVER : src[3 * ss + i];
  }
}

}  // namespace pe
