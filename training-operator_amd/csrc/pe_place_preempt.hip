// Place a batch, evicting as it goes (pe_place_preempt_domains): the placing frame of pe_place.hip -- one workgroup
// per active domain, the working state in LDS for segments of at most PL_LDS_NODES nodes and the compact global
// segment beyond -- with pe_preempt.hip's two phases run for every job that does not fit as things stand.
//
// ONE EVOLVING STATE.  pe_preempt.hip answers many independent pairs, so each judgement starts from a fresh copy of
// the segment and re-applies all of E.  Here the segment is the live state of a sequential batch and there is no
// pristine copy to return to; none is needed.  Every step is an integer add or subtract of the same numbers:
//   release(v)    += the records of victim v that name a node of the segment
//   take back(v)  -= the same records
//   an attempt    -= takes x requests, and a failed or undone attempt += exactly its logged takes (place_rollback)
// Two's-complement adds commute and cancel bit for bit, so after "release i .. attempt .. take back i" the state
// equals the state before in every cell, whatever happened in between, and the state a judgement at E sees equals a
// fresh copy plus E's records.  Phase 1 is therefore incremental (one victim's records per step, never the prefix
// again), phase 2 takes one victim's records off and puts them back on a failure, and a job costs its attempts and
// at most K + 2 (prefix - 1) record passes instead of K^2 / 2.
//
// A successful attempt STANDS (pods stored, residuals taken).  Phase 2 undoes the standing placement from its log
// before it tries without victim i; a try that succeeds stands in turn.  Only when the last try of phase 2 failed
// the job is placed once more against the final E (the state is the one that placed it before, so it is placed
// the same way).  A job that fits with nobody evicted costs one attempt, as in place_domains_kernel.
//
// Records are released by the threads striding over them with atomic adds between two barriers (two records may
// name one node, and a thread touches places that are not its own), pe_preempt.hip's default; DESIGN.md section
// 33 has the comparison with the owner adding its own.  vic_job[v] doubles as the DEAD flag of victim v: the plan
// refuses a victim listed in two domains, so one workgroup alone reads and writes the cell, thread 0 stores it and
// a barrier follows before any thread reads it again (an atomic load: the cell is never cached as read-only).
//
// place_preempt_sweep_kernel, launched after both instances: an evicted gang leaves whole, so its records on nodes
// outside the evicting job's segment go back to the live SoA -- after every job of the call is decided, so that no
// job saw them.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_place_step.h"
#include "pe_place_preempt_plan.h"

namespace pe {

namespace {

// The records of victim v that name a place of the segment [b, b + n), added to (sign +1) or taken off (-1) the
// working state w0[d * ws + place].  Called by the whole workgroup.
template <class Stride>
__device__ __forceinline__ void victim_records(int64_t* w0, Stride ws, int b, int n, const PlacePreIn& in, int v,
                                               int64_t sign) {
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  __syncthreads();   // the owners' takes of the last decision are done
  for (int r = in.rec_start[v] + (int)threadIdx.x; r < in.rec_start[v + 1]; r += PL_THREADS) {
    const uint64_t local = (uint64_t)(int64_t)in.recs[r].node - in.id_base;
    if (local >= (uint64_t)in.Ns) continue;
    const uint32_t at = (uint32_t)(in.node_place[local] - b);   // -1 or another segment's place: outside [0, n)
    if (at >= (uint32_t)n) continue;
    atomicAdd((unsigned long long*)&w0[at], (unsigned long long)(sign * in.recs[r].q[0]));
    atomicAdd((unsigned long long*)&w1[at], (unsigned long long)(sign * in.recs[r].q[1]));
    atomicAdd((unsigned long long*)&w2[at], (unsigned long long)(sign * in.recs[r].q[2]));
    atomicAdd((unsigned long long*)&w3[at], (unsigned long long)(sign * in.recs[r].q[3]));
  }
  __syncthreads();   // the owners read their places again
}

// place_job's (pe_place_job.h) walk, log and pod stores with the length of the log handed out, so that a placement
// that stands can be undone later as a failed one is at once: n_log entries at log[3 pod0 ..].
template <class Stride>
__device__ __forceinline__ bool attempt(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn, int& par,
                                        const PlaceGroup* __restrict__ groups, int g0, int g1,
                                        int32_t* __restrict__ out_pod, int32_t* __restrict__ log, int64_t& n_log) {
  const int tid = threadIdx.x;
  const int64_t pod0 = groups[g0].pod0;
  n_log = 0;
  uint32_t left;
  const bool ok = place_groups(r0, rs, gid, gid + rs, n, mn, par, groups, g0, g1, left,
                               [&](int g, const PlaceGroup& gr, const PlaceChoice& c, uint32_t done) {
                                 if (tid == 0) {
                                   int32_t* const e = log + 3 * (pod0 + n_log);
                                   e[0] = (int32_t)c.at;
                                   e[1] = g;
                                   e[2] = (int32_t)c.t;
                                 }
                                 ++n_log;
                                 const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
                                 const int64_t slot = gr.pod0 + done;
                                 for (int64_t p = slot + tid; p < slot + c.t; p += PL_THREADS) out_pod[p] = node;
                               }) == g1;
  return ok;
}

// What an attempt took comes back: its log's entries onto the state, its pod slots to -1.
template <class Stride>
__device__ __forceinline__ void undo(int64_t* r0, Stride rs, const PlaceGroup* __restrict__ groups, int g0, int g1,
                                     int32_t* __restrict__ out_pod, int32_t* __restrict__ log, int64_t n_log) {
  const int64_t pod0 = groups[g0].pod0;
  __syncthreads();   // the log's last entry and the last take are written
  place_rollback(r0, (int64_t)rs, groups, log + 3 * pod0, n_log, out_pod + pod0,
                 groups[g1 - 1].pod0 + groups[g1 - 1].count - pod0);
  __syncthreads();
}

// One domain's jobs jobs[j0 .. j1), in that order, on its n nodes at the places [b, b + n).
template <class Stride>
__device__ __forceinline__ void preempt_domain(int64_t* r0, const uint32_t* gid, Stride rs, int b, int n, PlaceMin& mn,
                                               const PlacePreIn& in, int j0, int j1, const PlacePreOut& out,
                                               int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  const PlaceGroup* const groups = in.groups;
  int par = 0;
  uint32_t attempts = 0;
  for (int ji = j0; ji < j1; ++ji) {
    const PreemptJob pj = in.jobs[ji];
    const int K = pj.v1 - pj.v0;   // <= 64
    const bool none = pj.g0 == pj.g1;   // no groups: placed as things stand
    int prefix = none ? 0 : -1;
    uint64_t E = 0;
    int64_t n_log = 0;
    // ONE loop with one attempt per turn, so that the decision (place_step.h) is instantiated once: turns of phase 1
    // (prefix k, one more live victim), then of phase 2 (position i comes off), then at most one turn that places
    // the job again after phase 2's last try failed
    bool phase2 = false, standing = false, again = false;
    int k = 0, i = -1;
    while (!none) {
      int v = -1;   // the victim whose records this turn moves
      if (!phase2) {
        if (k > K) break;   // every prefix failed
        if (k > 0) {
          v = in.list[pj.v0 + k - 1];   // < V: the plan validated the list
          const int32_t by = __builtin_amdgcn_readfirstlane(
              __hip_atomic_load(&out.vic_job[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
          if (by >= 0) {   // dead: releases nothing, and prefix k is not judged
            ++k;
            continue;
          }
          E |= 1ull << (k - 1);
        }
      } else {
        while (i >= 0 && !(E >> i & 1)) --i;   // live positions only; position prefix - 1 stays
        if (i >= 0) {
          v = in.list[pj.v0 + i];
        } else if (standing) {
          break;
        } else {
          again = true;   // the state that placed it before: placed again, the same way
        }
        if (standing) undo(r0, rs, groups, pj.g0, pj.g1, out.pod, log, n_log);
      }
      if (v >= 0) victim_records(r0, rs, b, n, in, v, phase2 ? -1 : 1);
      attempts += again ? 0 : 1;
      standing = attempt(r0, gid, rs, n, mn, par, groups, pj.g0, pj.g1, out.pod, log, n_log);
      if (!standing) undo(r0, rs, groups, pj.g0, pj.g1, out.pod, log, n_log);
      if (again) break;
      if (!phase2) {
        if (standing) {
          prefix = k;
          phase2 = true;
          i = k - 2;
        }
        ++k;
      } else {
        if (standing)
          E &= ~(1ull << i);
        else
          victim_records(r0, rs, b, n, in, v, 1);
        --i;
      }
    }
    if (prefix < 0) {   // nobody is evicted: the releases come off again
      for (uint64_t m = E; m != 0; m &= m - 1) victim_records(r0, rs, b, n, in, in.list[pj.v0 + __builtin_ctzll(m)], -1);
      E = 0;
    }
    if (tid == 0) {   // pj.job < J
      out.status[pj.job] = prefix < 0 ? 1 : 0;
      out.prefix[pj.job] = prefix;
      out.victims[pj.job] = E;
      for (uint64_t m = E; m != 0; m &= m - 1) out.vic_job[in.list[pj.v0 + __builtin_ctzll(m)]] = pj.job;
    }
    __syncthreads();   // the dead flags, before the next job reads them
  }
  if (tid == 0 && attempts) atomicAdd(out.attempts, (unsigned long long)attempts);
}

// pe_place_job.h's place_frame with the segment's first place handed to the body and the write-back left out of a
// dry run.  IN_LDS as for place_domains_kernel: two instances, each taking its kind of segment.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void place_preempt_kernel(PlacePreIn in, PlaceSegs sg, int64_t* __restrict__ res,
                                                                   int64_t stride, uint32_t id_base, int dry_run,
                                                                   PlacePreOut out, int32_t* __restrict__ log) {
  __shared__ PlaceMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= PL_LDS_NODES) != IN_LDS) return;
  int64_t* const g0 = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  const int j0 = in.job_start[a], j1 = in.job_start[a + 1];
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs) {
    preempt_domain(r0, ids, rs, b, n, mn, in, j0, j1, out, log);
    if (dry_run) return;
    for (int i = tid; i < n; i += PL_THREADS) {   // place i is its owner's, and the last barrier is behind
      const int64_t l = (int64_t)(ids[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
      for (int d = 0; d < D; ++d) res[d * stride + l] = r0[d * rs + i];
    }
  };
  if constexpr (IN_LDS) {
    __shared__ PlaceShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {
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

constexpr int SW_THREADS = 256, SW_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(SW_THREADS) void place_preempt_sweep_kernel(PlacePreIn in, int64_t V,
                                                                         const int32_t* __restrict__ seg_off,
                                                                         const int32_t* __restrict__ vic_job,
                                                                         int64_t* __restrict__ res, int64_t stride) {
  for (int64_t v = blockIdx.x; v < V; v += gridDim.x) {
    if (vic_job[v] < 0) continue;
    const int a = in.vic_act[v];   // >= 0: a job of that domain evicted it
    const int32_t lo = seg_off[a], hi = seg_off[a + 1];
    for (int r = in.rec_start[v] + (int)threadIdx.x; r < in.rec_start[v + 1]; r += SW_THREADS) {
      const uint64_t local = (uint64_t)(int64_t)in.recs[r].node - in.id_base;
      if (local >= (uint64_t)in.Ns) continue;
      const int32_t at = in.node_place[local];
      if (at >= lo && at < hi) continue;   // a place of the evicting job's segment: its workgroup gave it back
      if (res[local] == NEVER) continue;   // a removed slot
#pragma unroll
      for (int d = 0; d < D; ++d)   // two records, of any two victims, may name one node
        atomicAdd((unsigned long long*)&res[d * stride + local], (unsigned long long)in.recs[r].q[d]);
    }
  }
}

}  // namespace

hipError_t launch_place_preempt(hipStream_t s, const PlacePreIn& in, int A, const PlaceSegs& segs, int64_t* res,
                                int64_t stride, bool dry_run, const PlacePreOut& out, int32_t* log) {
  if (A <= 0) return hipSuccess;
  hipLaunchKernelGGL(place_preempt_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, in, segs, res, stride,
                     (uint32_t)in.id_base, (int)dry_run, out, log);
  hipLaunchKernelGGL(place_preempt_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, in, segs, res, stride,
                     (uint32_t)in.id_base, (int)dry_run, out, log);
  return hipGetLastError();
}

hipError_t launch_place_preempt_sweep(hipStream_t s, const PlacePreIn& in, int64_t V, const PlaceSegs& segs,
                                      const int32_t* vic_job, int64_t* res, int64_t stride) {
  if (V <= 0 || in.Ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(place_preempt_sweep_kernel, dim3((unsigned)std::min<int64_t>(V, SW_MAX_BLOCKS)), dim3(SW_THREADS), 0,
                     s, in, V, (const int32_t*)segs.seg_off, vic_job, res, stride);
  return hipGetLastError();
}

}  // namespace pe
