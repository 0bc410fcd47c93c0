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
// preempt_domains_kernel: units and instances as fit_domains_kernel -- one workgroup per unit of at most
// PRE_UNIT_PAIRS pairs with the working state in LDS for segments of at most PL_LDS_NODES nodes, private rows of
// the bounded global scratch (fit_scratch_layout) for larger ones.  R(E) is produced by re-applying E's records
// onto each fresh copy: the threads stride over the records of every victim of E and add each to its place with
// an atomic add (two records may name one node), between two barriers, since here a thread touches places that
// are not its own.  A judgement with E empty -- k = 0, the fit call's -- has neither.  Thread 0 stores the pair's
// three answers and lowers best[job] to count << 32 | pair (an unsigned 64-bit minimum over cells preset to ~0).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_step.h"
#include "pe_preempt_plan.h"

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
  const int tid = threadIdx.x;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  for (int i = tid; i < n; i += PL_THREADS) {   // a fresh copy, every thread its own places
    w0[i] = src[i];
    w1[i] = src[ss + i];
    w2[i] = src[2 * ss + i];
    w3[i] = src[3 * ss + i];
  }
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
  for (int g = pr.g0; g < pr.g1; ++g) {
    const PlaceGroup gr = in.groups[g];
    if (gr.count <= 0) continue;
    const bool unit = (gr.need & NEED_ISLAND) != 0;   // an island group: one decision for count x request
    int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
    if (unit && !island_request(gr, s0, s1, s2, s3)) return false;   // fits nowhere
    uint32_t left = (uint32_t)gr.count;
    while (left > 0) {
      const PlaceChoice c = place_decide(w0, w1, w2, w3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, left, mn, par);
      if (c.none()) return false;
      place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3);
      left -= c.t;
    }
  }
  return true;
}

// The pairs at places [p0, p1) of the plan's list, all of one segment, walked through the two phases.
template <class Stride>
__device__ __forceinline__ void preempt_pairs(int64_t* w0, Stride ws, const int64_t* __restrict__ src, int64_t ss,
                                              const uint32_t* gid, const uint32_t* lab, int b, int n, PlaceMin& mn,
                                              int& par, const PreIn& in, int p0, int p1, const PreOut& out) {
  for (int pi = p0; pi < p1; ++pi) {
    const PrePair pr = in.pairs[pi];
    const int K = pr.v1 - pr.v0;   // <= 64
    int prefix = -1;
    uint64_t E = 0;
    uint32_t judged = 0;
    for (int k = 0; k <= K && prefix < 0; ++k) {   // phase 1: the prefixes in ascending order
      E = k >= 64 ? ~0ull : (1ull << k) - 1;
      ++judged;
      if (judge(w0, ws, src, ss, gid, lab, b, n, mn, par, in, pr, E)) prefix = k;
    }
    if (prefix < 0) E = 0;
    for (int i = prefix - 2; i >= 0; --i) {   // phase 2: put back who was not needed; position prefix - 1 stays
      const uint64_t t = E & ~(1ull << i);
      ++judged;
      if (judge(w0, ws, src, ss, gid, lab, b, n, mn, par, in, pr, t)) E = t;
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
}

template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void preempt_domains_kernel(PreIn in, const FitLarge* __restrict__ large,
                                                                     int64_t* __restrict__ scratch,
                                                                     const int32_t* __restrict__ seg_off,
                                                                     const uint32_t* __restrict__ seg_gid,
                                                                     const uint32_t* __restrict__ seg_lab,
                                                                     const int64_t* __restrict__ seg_res, int64_t ss,
                                                                     PreOut out) {
  __shared__ PlaceMin mn;
  const int tid = threadIdx.x;
  int par = 0;
  if constexpr (IN_LDS) {
    const FitUnit u = in.units[blockIdx.x];
    const int b = seg_off[u.act], n = seg_off[u.act + 1] - b;
    if (n > PL_LDS_NODES) return;
    __shared__ PlaceShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
      sh.gid[i] = seg_gid[b + i];
      sh.lab[i] = seg_lab[b + i];
    }
    preempt_pairs(sh.r[0], std::integral_constant<int, PL_LDS_NODES>(), seg_res + b, ss, sh.gid, sh.lab, b, n, mn, par,
                  in, u.p0, u.p1, out);
  } else {
    const FitLarge w = large[blockIdx.x];
    const int b = seg_off[w.act], n = seg_off[w.act + 1] - b;
    for (int u = w.u0 + w.s; u < w.u1; u += w.k)   // the copy holds 4 n cells from w.at: the host laid it out for this n
      preempt_pairs(scratch + w.at, (int64_t)n, seg_res + b, ss, seg_gid + b, seg_lab + b, b, n, mn, par, in,
                    in.units[u].p0, in.units[u].p1, out);
  }
}

}  // namespace

hipError_t launch_preempt_place_map(hipStream_t s, const PlaceSegs& segs, int A, int64_t Ns, uint64_t id_base,
                                    int32_t* node_place) {
  if (A <= 0 || Ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(preempt_place_map_kernel, dim3((unsigned)((Ns + 255) / 256)), dim3(256), 0, s,
                     (const int32_t*)segs.seg_off, A, (const uint32_t*)segs.gid, Ns, id_base, node_place);
  return hipGetLastError();
}

hipError_t launch_preempt_units(hipStream_t s, const PreIn& in, int64_t U, const PlaceSegs& segs, const PreOut& out) {
  if (U <= 0) return hipSuccess;
  if (U > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(preempt_domains_kernel<true>, dim3((unsigned)U), dim3(PL_THREADS), 0, s, in, (const FitLarge*)nullptr,
                     (int64_t*)nullptr, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid, (const uint32_t*)segs.lab,
                     (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

hipError_t launch_preempt_large(hipStream_t s, const PreIn& in, const FitLarge* large, int64_t n_large, int64_t* scratch,
                                const PlaceSegs& segs, const PreOut& out) {
  if (n_large <= 0) return hipSuccess;
  if (n_large > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(preempt_domains_kernel<false>, dim3((unsigned)n_large), dim3(PL_THREADS), 0, s, in, large, scratch,
                     (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid, (const uint32_t*)segs.lab,
                     (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
