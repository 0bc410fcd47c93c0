// Which gangs must go for a gang to fit (pe_gang_preempt_domains): per (job, domain) pair with an ordered list
// of candidate victims, the smallest prefix of the list whose release lets the job be placed in the domain, then
// the fill-back that returns the victims that were not needed.  Every step is one JUDGEMENT, pe_fit.hip's: a
// fresh copy of the domain's segment, here plus the releases of a set E of list positions, and the job's groups
// through the placement's decision (pe_place_step.h) until a pod finds no node.  The rule is not monotone in the
// residuals, so the prefixes are walked in ascending order and nothing is bisected.
//
// Member lists: pe_place.hip's launch_place_members, read-only.  preempt_place_map_kernel inverts them: the
// place of every node in the segments' arrays, so that a release record (node, request x run) finds its place in
// the working state; a node of no active domain keeps -1 and its records count nothing.
//
// preempt_domains_kernel: the what-if frame (pe_what_if.h), as fit_domains_kernel -- one workgroup per unit of at
// most PRE_UNIT_PAIRS pairs with the working state in LDS for segments of at most PL_LDS_NODES nodes, private rows
// of the bounded global scratch (fit_scratch_layout) for larger ones -- around this file's own lines: the two
// phases of a pair and, in judge, the releases between the fresh copy (what_if_copy) and the groups' walk
// (place_groups, pe_place_step.h).  R(E) is produced by re-applying E's records
// onto each fresh copy: the threads stride over the records of every victim of E and add each to its place with
// an atomic add (two records may name one node), between two barriers, since here a thread touches places that
// are not its own.  A judgement with E empty -- k = 0, the fit call's -- has neither.  Thread 0 stores the pair's
// three answers and lowers best[job] to count << 32 | pair (an unsigned 64-bit minimum over cells preset to ~0).
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_preempt_plan.h"
#include "pe_what_if.h"

namespace pe {

namespace {

__global__ __launch_bounds__(256) void preempt_place_map_kernel(const int32_t* __restrict__ seg_off, int A,
                                                                const uint32_t* __restrict__ seg_gid, int64_t Ns,
                                                                uint64_t id_base, int32_t* __restrict__ node_place) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= Ns || s >= seg_off[A]) return;   // the segments hold at most Ns places
  const uint64_t local = (uint64_t)seg_gid[s] - id_base;
  if (local < (uint64_t)Ns) node_place[local] = (int32_t)s;
}

// One judgement: would the job of `pr` be placed on the segment (n nodes at places [b, b + n) of the segments'
// arrays, residuals src) with the victims at the positions of E released?  The same on every thread.
template <class Stride>
__device__ __forceinline__ bool judge(int64_t* w0, Stride ws, const int64_t* __restrict__ src, int64_t ss,
                                      const uint32_t* gid, const uint32_t* lab, int b, int n, PlaceMin& mn, int& par,
                                      const PreIn& in, const PrePair& pr, uint64_t E) {
  what_if_copy(w0, ws, src, ss, n);
  const int tid = threadIdx.x;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
#ifdef PE_PREEMPT_OWNER_ADDS
  // (A/B build) every thread reads all of E's records and adds those of its own places: no
  // barrier and no atomic, |records| loads per thread instead of |records| / PL_THREADS
  for (uint64_t m = E; m != 0; m &= m - 1) {
    const int v = in.list[pr.v0 + __builtin_ctzll(m)];
    for (int r = in.rec_start[v]; r < in.rec_start[v + 1]; ++r) {
      const uint64_t local = (uint64_t)(int64_t)in.recs[r].node - in.id_base;
      if (local >= (uint64_t)in.Ns) continue;
      const uint32_t at = (uint32_t)(in.node_place[local] - b);
      if (at >= (uint32_t)n || (at & (PL_THREADS - 1)) != (uint32_t)tid) continue;
      w0[at] += in.recs[r].q[0];
      w1[at] += in.recs[r].q[1];
      w2[at] += in.recs[r].q[2];
      w3[at] += in.recs[r].q[3];
    }
  }
#else
  if (E != 0) {   // the releases: any thread, any place
    __syncthreads();
    for (uint64_t m = E; m != 0; m &= m - 1) {
      const int v = in.list[pr.v0 + __builtin_ctzll(m)];   // < V: the plan validated the list
      for (int r = in.rec_start[v] + tid; r < in.rec_start[v + 1]; r += PL_THREADS) {
        const uint64_t local = (uint64_t)(int64_t)in.recs[r].node - in.id_base;
        if (local >= (uint64_t)in.Ns) continue;
        const uint32_t at = (uint32_t)(in.node_place[local] - b);   // -1 or another segment's place: outside [0, n)
        if (at >= (uint32_t)n) continue;
        atomicAdd((unsigned long long*)&w0[at], (unsigned long long)in.recs[r].q[0]);
        atomicAdd((unsigned long long*)&w1[at], (unsigned long long)in.recs[r].q[1]);
        atomicAdd((unsigned long long*)&w2[at], (unsigned long long)in.recs[r].q[2]);
        atomicAdd((unsigned long long*)&w3[at], (unsigned long long)in.recs[r].q[3]);
      }
    }
    __syncthreads();
  }
#endif
  uint32_t left;   // (>=: with == the global instance parks one more SGPR in a VGPR lane)
  return place_groups(w0, ws, gid, lab, n, mn, par, in.groups, pr.g0, pr.g1, left,
                      [](int, const PlaceGroup&, const PlaceChoice&, uint32_t) {}) >= pr.g1;
}

// what_if_units' body: the pairs at places [p0, p1) of the plan's list, all of one segment, walked through the two
// phases.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void preempt_domains_kernel(PreIn in, const FitLarge* __restrict__ large,
                                                                     int64_t* __restrict__ scratch,
                                                                     const int32_t* __restrict__ seg_off,
                                                                     const uint32_t* __restrict__ seg_gid,
                                                                     const uint32_t* __restrict__ seg_lab,
                                                                     const int64_t* __restrict__ seg_res, int64_t ss,
                                                                     PreOut out) {
  what_if_units<IN_LDS>(
      in.units, large, scratch, seg_off, seg_gid, seg_lab, seg_res, ss,
      [&](int64_t* w0, auto ws, const int64_t* src, int64_t rs, const uint32_t* gid, const uint32_t* lab, int b, int n,
          PlaceMin& mn, int& par, int p0, int p1) {
        for (int pi = p0; pi < p1; ++pi) {
          const PrePair pr = in.pairs[pi];
          const int K = pr.v1 - pr.v0;   // <= 64
          int prefix = -1;
          uint64_t E = 0;
          uint32_t judged = 0;
          for (int k = 0; k <= K && prefix < 0; ++k) {   // phase 1: the prefixes in ascending order
            E = k >= 64 ? ~0ull : (1ull << k) - 1;
            ++judged;
            if (judge(w0, ws, src, rs, gid, lab, b, n, mn, par, in, pr, E)) prefix = k;
          }
          if (prefix < 0) E = 0;
          for (int i = prefix - 2; i >= 0; --i) {   // phase 2: put back who was not needed; position prefix - 1 stays
            const uint64_t t = E & ~(1ull << i);
            ++judged;
            if (judge(w0, ws, src, rs, gid, lab, b, n, mn, par, in, pr, t)) E = t;
          }
          if (threadIdx.x == 0) {   // pr.pair < P, pr.job < J: the plan validated the list
            const int count = prefix < 0 ? -1 : __builtin_popcountll(E);
            out.prefix[pr.pair] = prefix;
            out.victims[pr.pair] = E;
            out.count[pr.pair] = count;
            if (prefix >= 0) atomicMin(&out.best[pr.job], (unsigned long long)count << 32 | (uint32_t)pr.pair);
            atomicAdd(out.judged, (unsigned long long)judged);
          }
        }
      });
}

}  // namespace

hipError_t launch_preempt_place_map(hipStream_t s, const PlaceSegs& segs, int A, int64_t Ns, uint64_t id_base,
                                    int32_t* node_place) {
  if (A <= 0 || Ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(preempt_place_map_kernel, dim3((unsigned)((Ns + 255) / 256)), dim3(256), 0, s,
                     (const int32_t*)segs.seg_off, A, (const uint32_t*)segs.gid, Ns, id_base, node_place);
  return hipGetLastError();
}

hipError_t launch_preempt(hipStream_t s, const PreIn& in, int64_t blocks, const FitLarge* large, int64_t* scratch,
                          const PlaceSegs& segs, const PreOut& out) {
  if (blocks <= 0) return hipSuccess;
  if (blocks > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(large ? preempt_domains_kernel<false> : preempt_domains_kernel<true>, dim3((unsigned)blocks),
                     dim3(PL_THREADS), 0, s, in, large, scratch, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid,
                     (const uint32_t*)segs.lab, (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
