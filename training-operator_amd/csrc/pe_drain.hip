// Can a node's pods move elsewhere, and where (pe_drain_fit_domains): would pe_place_greedy_domains, given the pods
// that sit on a candidate node as one job in a chosen domain, place them on the domain's OTHER nodes against the
// current residuals?  Every candidate is judged alone, so the work is the fit call's (pe_fit.hip): the plan
// (pe_drain_plan.h) turns a candidate's pods into the runs of one synthetic job, cuts each active domain's
// candidates into WORK UNITS of at most FIT_UNIT_PAIRS, and one workgroup per unit judges its candidates one after
// the other.
//
// drain_domains_kernel: the what-if frame (pe_what_if.h) and the groups' walk (pe_place_step.h), as in
// fit_domains_kernel, around this file's own lines, which are two.  The fresh copy of the segment's four residual
// rows writes NEVER into all four rows of the place whose id is the candidate's node (what_if_copy<true>) -- what
// a removed slot holds, so that no request, not even a zero one, fits it.  The thread that copies place i is
// the only one that ever touches it, so the exclusion needs no barrier, and the next candidate's copy undoes it.
// The STORE instances also say where every pod goes: as a take of t pods is made, target[slot_list[...]] of the
// run's next t slots receives the chosen node, and a candidate that fails has -1 written back over all its slots.
// Place p of a candidate's slots is written by thread p mod PL_THREADS in both cases, so the -1 follows the node
// in program order and needs no barrier either.  Thread 0 stores the candidate's three answers.  Plain vector
// stores only.
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_what_if.h"

namespace pe {

namespace {

// what_if_units' body: per candidate a fresh copy without its node, its runs through the walk (a run's count is
// >= 1: the plan makes no empty run), the targets, the three answers.
template <bool IN_LDS, bool STORE>
__global__ __launch_bounds__(PL_THREADS) void drain_domains_kernel(
    const PlaceGroup* __restrict__ runs, const DrainPair* __restrict__ pairs, const FitUnit* __restrict__ units,
    const FitLarge* __restrict__ large, int64_t* __restrict__ scratch, const int32_t* __restrict__ slot_list,
    const int32_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_gid, const uint32_t* __restrict__ seg_lab,
    const int64_t* __restrict__ seg_res, int64_t ss, DrainOut out) {
  what_if_units<IN_LDS>(
      units, large, scratch, seg_off, seg_gid, seg_lab, seg_res, ss,
      [&](int64_t* w0, auto ws, const int64_t* src, int64_t rs, const uint32_t* gid, const uint32_t* lab, int, int n,
          PlaceMin& mn, int& par, int p0, int p1) {
        const int tid = threadIdx.x;
        for (int pi = p0; pi < p1; ++pi) {
          const DrainPair pr = pairs[pi];
          what_if_copy<true>(w0, ws, src, rs, n, gid, (uint32_t)pr.node);
          // the candidate's slots: places [c0, c1) of the slot list, its runs back to back
          const int64_t c0 = pr.g0 < pr.g1 ? runs[pr.g0].pod0 : 0;
          int64_t moved = 0;   // pods the rule has placed so far
          uint32_t left;
          const int g = place_groups(
              w0, ws, gid, lab, n, mn, par, runs, pr.g0, pr.g1, left,
              [&](int, const PlaceGroup& gr, const PlaceChoice& c, uint32_t done) {
                if constexpr (STORE) {
                  const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
                  const int64_t b = gr.pod0 + (int64_t)done - c0;   // the take's first place, from c0
                  for (int64_t p = b + (((int64_t)tid - b) & (PL_THREADS - 1)); p < b + c.t; p += PL_THREADS)
                    out.target[slot_list[c0 + p]] = node;   // c0 + p < c1 <= E, every slot < S: the plan's lists
                }
                moved += c.t;
              });
          // the place in the slot list of the first pod that found no node: an island run fails as a whole, with
          // all its pods left
          const int64_t fail_at = g < pr.g1 ? runs[g].pod0 + (int64_t)((uint32_t)runs[g].count - left) : -1;
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
      });
}

}  // namespace

hipError_t launch_drain(hipStream_t s, const PlaceGroup* runs, const DrainPair* pairs, const FitUnit* units, int64_t blocks,
                        const FitLarge* large, int64_t* scratch, const int32_t* slot_list, const PlaceSegs& segs,
                        const DrainOut& out, bool store) {
  if (blocks <= 0) return hipSuccess;
  if (blocks > (int64_t)INT32_MAX || (store && !out.target)) return hipErrorInvalidValue;
  const auto kernel = large ? (store ? drain_domains_kernel<false, true> : drain_domains_kernel<false, false>)
                            : (store ? drain_domains_kernel<true, true> : drain_domains_kernel<true, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(PL_THREADS), 0, s, runs, pairs, units, large, scratch, slot_list,
                     (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid, (const uint32_t*)segs.lab,
                     (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
