// Can a node's pods move elsewhere, and where (pe_drain_fit_domains): would pe_place_greedy_domains, given the pods
// that sit on a candidate node as one job in a chosen domain, place them on the domain's OTHER nodes against the
// current residuals?  Every candidate is judged alone, so the work is the fit call's (pe_fit.hip): the plan
// (pe_drain_plan.h) turns a candidate's pods into the runs of one synthetic job, cuts each active domain's
// candidates into WORK UNITS of at most FIT_UNIT_PAIRS, and one workgroup per unit judges its candidates one after
// the other.
//
// drain_domains_kernel: fit_domains_kernel's loop with two additions.  The copy of the segment's four residual
// rows into the working state writes NEVER into all four rows of the place whose id is the candidate's node --
// what a removed slot holds, so that no request, not even a zero one, fits it.  The thread that copies place i is
// the only one that ever touches it, so the exclusion needs no barrier, and the next candidate's copy undoes it.
// The STORE instances also say where every pod goes: as a take of t pods is made, target[slot_list[...]] of the
// run's next t slots receives the chosen node, and a candidate that fails has -1 written back over all its slots.
// Place p of a candidate's slots is written by thread p mod PL_THREADS in both cases, so the -1 follows the node
// in program order and needs no barrier either.  Thread 0 stores the candidate's three answers.  Working state,
// staging and the two instances per STORE are the fit kernel's: LDS up to PL_LDS_NODES nodes, a private copy in a
// global scratch array (pe_fit_plan.h fit_scratch_layout) beyond.  Plain vector stores only.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_fit_plan.h"
#include "pe_kernels.h"
#include "pe_place_step.h"

namespace pe {

namespace {

// The candidates at places [p0, p1) of the plan's list, all of one segment: n nodes with ids gid[i], labels lab[i]
// and residuals src[d * ss + i] (read), judged on the working state w0[d * ws + i] (written).
template <bool STORE, class Stride>
__device__ __forceinline__ void drain_pairs(int64_t* w0, Stride ws, const int64_t* __restrict__ src, int64_t ss,
                                            const uint32_t* gid, const uint32_t* lab, int n, PlaceMin& mn, int& par,
                                            const PlaceGroup* __restrict__ runs, const DrainPair* __restrict__ pairs,
                                            int p0, int p1, const int32_t* __restrict__ slot_list, const DrainOut& out) {
  const int tid = threadIdx.x;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  for (int pi = p0; pi < p1; ++pi) {
    const DrainPair pr = pairs[pi];
    const uint32_t gone = (uint32_t)pr.node;
    for (int i = tid; i < n; i += PL_THREADS) {   // a fresh copy without the candidate's node
      const bool out_of_it = gid[i] == gone;
      w0[i] = out_of_it ? NEVER : src[i];
      w1[i] = out_of_it ? NEVER : src[ss + i];
      w2[i] = out_of_it ? NEVER : src[2 * ss + i];
      w3[i] = out_of_it ? NEVER : src[3 * ss + i];
    }
    // the candidate's slots: places [c0, c1) of the slot list, its runs back to back
    const int64_t c0 = pr.g0 < pr.g1 ? runs[pr.g0].pod0 : 0;
    int64_t moved = 0;      // pods the rule has placed so far
    int64_t fail_at = -1;   // the place in the slot list of the first pod that found no node
    for (int g = pr.g0; g < pr.g1 && fail_at < 0; ++g) {
      const PlaceGroup gr = runs[g];   // gr.count >= 1: the plan makes no empty run
      const bool unit = (gr.need & NEED_ISLAND) != 0;   // an island run: one decision for count x request
      int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
      if (unit && !island_request(gr, s0, s1, s2, s3)) {   // fits nowhere
        fail_at = gr.pod0;
        break;
      }
      uint32_t left = (uint32_t)gr.count;
      while (left > 0) {
        const PlaceChoice c = place_decide(w0, w1, w2, w3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, left, mn, par);
        if (c.none()) {   // no node of the domain fits
          fail_at = unit ? gr.pod0 : gr.pod0 + (int64_t)((uint32_t)gr.count - left);
          break;
        }
        place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3);
        if constexpr (STORE) {
          const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
          const int64_t b = gr.pod0 + (int64_t)((uint32_t)gr.count - left) - c0;   // the take's first place, from c0
          for (int64_t p = b + (((int64_t)tid - b) & (PL_THREADS - 1)); p < b + c.t; p += PL_THREADS)
            out.target[slot_list[c0 + p]] = node;   // c0 + p < c1 <= E, every slot < S: the plan's lists
        }
        moved += c.t;
        left -= c.t;
      }
    }
    if constexpr (STORE) {
      if (fail_at >= 0) {   // (then the candidate has a run)
        const int64_t c1 = runs[pr.g1 - 1].pod0 + runs[pr.g1 - 1].count;
        for (int64_t p = tid; p < c1 - c0; p += PL_THREADS) out.target[slot_list[c0 + p]] = -1;
      }
    }
    if (tid == 0) {   // pr.cand < C: the plan validated the list
      out.fits[pr.cand] = fail_at < 0;
      out.moved[pr.cand] = moved;
      out.fail_slot[pr.cand] = fail_at < 0 ? -1 : (int64_t)slot_list[fail_at];
    }
  }
}

// IN_LDS: one workgroup per unit, for the units whose segment has at most PL_LDS_NODES nodes (a workgroup whose
// segment is larger leaves at once); the other instance has one workgroup per FitLarge record.
template <bool IN_LDS, bool STORE>
__global__ __launch_bounds__(PL_THREADS) void drain_domains_kernel(
    const PlaceGroup* __restrict__ runs, const DrainPair* __restrict__ pairs, const FitUnit* __restrict__ units,
    const FitLarge* __restrict__ large, int64_t* __restrict__ scratch, const int32_t* __restrict__ slot_list,
    const int32_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_gid, const uint32_t* __restrict__ seg_lab,
    const int64_t* __restrict__ seg_res, int64_t ss, DrainOut out) {
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
    drain_pairs<STORE>(sh.r[0], std::integral_constant<int, PL_LDS_NODES>(), seg_res + b, ss, sh.gid, sh.lab, n, mn, par,
                       runs, pairs, u.p0, u.p1, slot_list, out);
  } else {
    const FitLarge w = large[blockIdx.x];
    const int b = seg_off[w.act], n = seg_off[w.act + 1] - b;
    for (int u = w.u0 + w.s; u < w.u1; u += w.k)   // the copy holds 4 n cells from w.at: the host laid it out for this n
      drain_pairs<STORE>(scratch + w.at, (int64_t)n, seg_res + b, ss, seg_gid + b, seg_lab + b, n, mn, par, runs, pairs,
                         units[u].p0, units[u].p1, slot_list, out);
  }
}

template <bool IN_LDS, bool STORE>
void drain_launch(hipStream_t s, unsigned blocks, const PlaceGroup* runs, const DrainPair* pairs, const FitUnit* units,
                  const FitLarge* large, int64_t* scratch, const int32_t* slot_list, const PlaceSegs& segs,
                  const DrainOut& out) {
  hipLaunchKernelGGL((drain_domains_kernel<IN_LDS, STORE>), dim3(blocks), dim3(PL_THREADS), 0, s, runs, pairs, units, large,
                     scratch, slot_list, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid, (const uint32_t*)segs.lab,
                     (const int64_t*)segs.res, segs.seg_stride, out);
}

}  // namespace

hipError_t launch_drain_units(hipStream_t s, const PlaceGroup* runs, const DrainPair* pairs, const FitUnit* units,
                              int64_t U, const int32_t* slot_list, const PlaceSegs& segs, const DrainOut& out, bool store) {
  if (U <= 0) return hipSuccess;
  if (U > (int64_t)INT32_MAX || (store && !out.target)) return hipErrorInvalidValue;
  if (store)
    drain_launch<true, true>(s, (unsigned)U, runs, pairs, units, nullptr, nullptr, slot_list, segs, out);
  else
    drain_launch<true, false>(s, (unsigned)U, runs, pairs, units, nullptr, nullptr, slot_list, segs, out);
  return hipGetLastError();
}

hipError_t launch_drain_large(hipStream_t s, const PlaceGroup* runs, const DrainPair* pairs, const FitUnit* units,
                              const FitLarge* large, int64_t n_large, int64_t* scratch, const int32_t* slot_list,
                              const PlaceSegs& segs, const DrainOut& out, bool store) {
  if (n_large <= 0) return hipSuccess;
  if (n_large > (int64_t)INT32_MAX || (store && !out.target)) return hipErrorInvalidValue;
  if (store)
    drain_launch<false, true>(s, (unsigned)n_large, runs, pairs, units, large, scratch, slot_list, segs, out);
  else
    drain_launch<false, false>(s, (unsigned)n_large, runs, pairs, units, large, scratch, slot_list, segs, out);
  return hipGetLastError();
}

}  // namespace pe
