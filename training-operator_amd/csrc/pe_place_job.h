// What the placing kernels share (device code only).  place_job: one job of the Appendix-B rule on a domain's
// segment, all or nothing -- pe_place_step.h's walk with this file's log of takes, pod stores and rollback -- for
// pe_place.hip (pe_place_greedy_domains, pe_place_first_fit_domains) and pe_place_min.hip (phase 1 of
// pe_place_min_member_domains).  place_frame: stage a domain's segment, run its jobs, write the residuals back,
// for place_domains_kernel and place_min_domains_kernel (first_fit_round_kernel stages lazily and writes back to
// the segment: a frame of its own, in pe_place.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_step.h"

namespace pe {

namespace {

// A failed job gives back what it took: its n_log log entries (place, group, pods) added back to the working
// state r[d * rs + place] and its n_pods pod slots set to -1.  Out of line, on generic pointers (the state is in
// LDS or global memory): the path is cold, and inlined its uniform values cost the decision loop SGPRs.
__device__ __noinline__ void place_rollback(int64_t* r, int64_t rs, const PlaceGroup* __restrict__ groups,
                                            const int32_t* __restrict__ entries, int64_t n_log, int32_t* __restrict__ pods,
                                            int64_t n_pods) {
  const int tid = threadIdx.x;
  for (int64_t e = tid; e < n_log; e += PL_THREADS) {
    const int32_t* const en = entries + 3 * e;
    const int64_t t = en[2];
    const PlaceGroup& gr = groups[en[1]];
    int64_t* const at = r + en[0];   // a place of the segment: the decision wrote it
#pragma unroll
    for (int d = 0; d < D; ++d)   // two entries may name one node: atomic
      atomicAdd((unsigned long long*)(at + d * rs), (unsigned long long)(t * gr.q[d]));
  }
  for (int64_t p = tid; p < n_pods; p += PL_THREADS) pods[p] = -1;
}

// One job (groups [g0, g1), g0 < g1) on a domain's n nodes, whose working state is r[d * rs + i] (written), gid[i]
// and labels gid[rs + i]: whether it is placed, the same on every thread.  A job that is not gives back what it
// took before the call returns.  `par`: place_decide's, carried from job to job.
template <class Stride>
__device__ __forceinline__ bool place_job(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn, int& par,
                                          const PlaceGroup* __restrict__ groups, int g0, int g1,
                                          int32_t* __restrict__ out_pod, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  // log entry e, three words at log[3 e]: its place in the segment, its group, the pods it placed
  const int64_t pod0 = groups[g0].pod0;   // the job's pod slots: [pod0, the last group's pod0 + count)
  int64_t n_log = 0;   // entries of this job, at log[pod0 ..]; <= the pods it placed
  uint32_t left;
  const bool ok =
      place_groups(r0, rs, gid, gid + rs, n, mn, par, groups, g0, g1, left,
                   [&](int g, const PlaceGroup& gr, const PlaceChoice& c, uint32_t done) {
                     if (tid == 0) {   // n_log < the pods the job placed so far, this decision's included
                       int32_t* const e = log + 3 * (pod0 + n_log);
                       e[0] = (int32_t)c.at;
                       e[1] = g;
                       e[2] = (int32_t)c.t;
                     }
                     ++n_log;
                     const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
                     const int64_t slot = gr.pod0 + done;   // slot + t <= pod1 <= P
                     for (int64_t p = slot + tid; p < slot + c.t; p += PL_THREADS) out_pod[p] = node;
                   }) == g1;
  if (!ok) {
    // every update and pod store of this job lies before the barrier of the decision that failed -- or,
    // for an overflowing island group, before this one
    __syncthreads();
    place_rollback(r0, (int64_t)rs, groups, log + 3 * pod0, n_log, out_pod + pod0,
                   groups[g1 - 1].pod0 + groups[g1 - 1].count - pod0);
    __syncthreads();   // the owners read their places again
  }
  return ok;
}

// The frame of a placing kernel, one workgroup per active domain a = blockIdx.x: the IN_LDS instance stages the
// segments of at most PL_LDS_NODES nodes in LDS -- four residual rows, labels, ids -- and the other instance works
// on the larger ones in place (a workgroup whose segment is the other instance's leaves at once); then
// body(r0, gid, rs, n, mn) runs the domain's jobs on that working state, and the residuals go back to the live
// SoA res[d * stride + id - id_base].
template <bool IN_LDS, class Body>
__device__ __forceinline__ void place_frame(const PlaceSegs& sg, int64_t* __restrict__ res, int64_t stride,
                                            uint32_t id_base, Body&& body) {
  __shared__ PlaceMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= PL_LDS_NODES) != IN_LDS) return;
  int64_t* const g0 = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs) {
    body(r0, ids, rs, n, mn);
    for (int i = tid; i < n; i += PL_THREADS) {
      const int64_t l = (int64_t)(ids[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
      for (int d = 0; d < D; ++d) res[d * stride + l] = r0[d * rs + i];
    }
  };
  if constexpr (IN_LDS) {
    __shared__ PlaceShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
#pragma unroll
      for (int d = 0; d < D; ++d) sh.r[d][i] = g0[d * ss + i];
      sh.lab[i] = gid[ss + i];
      sh.gid[i] = gid[i];
    }
    run(sh.r[0], sh.gid, std::integral_constant<int, PL_LDS_NODES>());
  } else {
    run(g0, gid, ss);
  }
}

}  // namespace

}  // namespace pe
