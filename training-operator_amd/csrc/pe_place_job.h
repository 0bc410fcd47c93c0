// One job of the Appendix-B rule on a domain's segment, with its rollback: the all-or-nothing loop shared by
// pe_place.hip (pe_place_greedy_domains, pe_place_first_fit_domains) and pe_place_min.hip (phase 1 of
// pe_place_min_member_domains).  Device code only; the decision itself is pe_place_step.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
  int64_t* const r1 = r0 + rs;
  int64_t* const r2 = r1 + rs;
  int64_t* const r3 = r2 + rs;
  const uint32_t* const lab = gid + rs;
  // log entry e, three words at log[3 e]: its place in the segment, its group, the pods it placed
  const int64_t pod0 = groups[g0].pod0;   // the job's pod slots: [pod0, the last group's pod0 + count)
  int64_t n_log = 0;   // entries of this job, at log[pod0 ..]; <= the pods it placed
  bool ok = true;
  for (int g = g0; g < g1 && ok; ++g) {
    const PlaceGroup gr = groups[g];
    if (gr.count <= 0) continue;
    const bool unit = (gr.need & NEED_ISLAND) != 0;   // an island group: one decision for count x request
    int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];   // the request the scan scores
    if (unit && !island_request(gr, s0, s1, s2, s3)) {   // fits nowhere
      ok = false;
      break;
    }
    uint32_t left = (uint32_t)gr.count;
    int64_t slot = gr.pod0;
    while (left > 0) {
      const PlaceChoice c = place_decide(r0, r1, r2, r3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, left, mn, par);
      if (c.none()) {   // no node of the domain fits
        ok = false;
        break;
      }
      place_take(r0, r1, r2, r3, c, unit, s0, s1, s2, s3);
      const uint32_t at = c.at, t = c.t;
      if (tid == 0) {   // n_log < the pods the job placed so far, this decision's included
        int32_t* const e = log + 3 * (pod0 + n_log);
        e[0] = (int32_t)at;
        e[1] = g;
        e[2] = (int32_t)t;
      }
      ++n_log;
      const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
      for (int64_t p = slot + tid; p < slot + t; p += PL_THREADS) out_pod[p] = node;   // slot + t <= pod1 <= P
      slot += t;
      left -= t;
    }
  }
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

}  // namespace

}  // namespace pe
