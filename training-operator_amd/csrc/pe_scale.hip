// Fewest new nodes for a gang to fit a domain (pe_scale_up_domains): how many nodes of a template would have to
// join the domain for pe_place_greedy_domains, given this one job in this domain against the current residuals, to
// place it?  Every (job, domain, template) pair is judged alone, so the work is the fit call's (pe_fit.hip) times
// the attempts: the plan (pe_scale_plan.h) cuts each active domain's pairs into WORK UNITS by the attempts they may
// cost, and one workgroup per unit walks its pairs one after the other.
//
// scale_domains_kernel: the what-if frame (pe_what_if.h) and the groups' walk (pe_place_step.h), as in
// fit_domains_kernel, around this file's own lines.  Attempt k = 0, 1, ... kmax of a pair is one judgement on the
// segment's n places and k NEW PLACES that are in no segment: the walk's second span (pe_place_step.h; NewPlaces
// below), new place j in the registers of thread j -- at most PE_MAX_SCALE_NODES = 64 of them, so no LDS beyond
// fit_domains_kernel's and four workgroups per CU as there.  Every attempt begins with a fresh copy of the
// segment's four residual rows and a fresh fill of the new places from the pair's template; thread i mod PL_THREADS
// is the only one that touches place i of either span, so neither needs a barrier, and a decision costs the one
// barrier it always did.  The answer is NOT monotone in k, so the attempts run in ascending
// order and stop at the first that places the job; the deciding attempt -- that one, or attempt kmax -- leaves
// its answers in the walk's variables, and thread 0 stores them and lowers best[job] to (nodes, pair) by an
// unsigned 64-bit minimum over cells the host set to ~0.  Plain vector stores only.
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_what_if.h"

namespace pe {

namespace {

// The new places of one attempt as the walk's second span: thread j holds new place j -- residual x0 .. x3, labels
// and id -- and `live` says whether attempt k has it (j < k).
struct NewPlaces {
  static constexpr bool present = true;
  int64_t x0, x1, x2, x3;
  uint32_t lab, gid;
  bool live;
};

// what_if_units' body: per pair the attempts in ascending order, each a fresh copy, a fresh fill and the job's
// groups through the walk; then the deciding attempt's answers.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void scale_domains_kernel(ScaleIn in, const FitLarge* __restrict__ large,
                                                                   int64_t* __restrict__ scratch,
                                                                   const int32_t* __restrict__ seg_off,
                                                                   const uint32_t* __restrict__ seg_gid,
                                                                   const uint32_t* __restrict__ seg_lab,
                                                                   const int64_t* __restrict__ seg_res, int64_t ss,
                                                                   ScaleOut out) {
  what_if_units<IN_LDS>(
      in.units, large, scratch, seg_off, seg_gid, seg_lab, seg_res, ss,
      [&](int64_t* w0, auto ws, const int64_t* src, int64_t rs, const uint32_t* gid, const uint32_t* lab, int, int n,
          PlaceMin& mn, int& par, int p0, int p1) {
        const int tid = threadIdx.x;
        NewPlaces fresh;
        fresh.gid = tid < in.n_new ? (uint32_t)in.new_slot[tid] : 0u;   // n_new <= 64: the host checked
        for (int pi = p0; pi < p1; ++pi) {
          const ScalePair pr = in.pairs[pi];
          const int64_t* const t = in.tmpl_res + 4 * (int64_t)pr.tmpl;   // pr.tmpl < T: the plan validated the list
          const int64_t t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
          fresh.lab = in.tmpl_lab[pr.tmpl];
          int nodes = -1, fail = -1;
          int64_t placed = 0, on_new = 0;   // the deciding attempt's: pods placed, and those of them on new places
          for (int k = 0; k <= pr.kmax && nodes < 0; ++k) {   // kmax <= n_new
            what_if_copy(w0, ws, src, rs, n);   // every attempt starts from fresh residuals, real ...
            fresh.x0 = t0;                      // ... and new
            fresh.x1 = t1;
            fresh.x2 = t2;
            fresh.x3 = t3;
            fresh.live = tid < k;
            placed = 0;
            on_new = 0;
            uint32_t left;
            const int g = place_groups(
                w0, ws, gid, lab, n, mn, par, in.groups, pr.g0, pr.g1, left,
                [&](int, const PlaceGroup&, const PlaceChoice& c, uint32_t) {
                  placed += c.t;
                  if (c.at >= (uint32_t)n) on_new += c.t;
                },
                fresh);
            fail = g < pr.g1 ? g - pr.g0 : -1;   // the first group, from the job's first, not placed in full
            if (fail < 0) nodes = k;
          }
          if (tid == 0) {   // pr.pair < P, pr.job < J: the plan validated the list
            out.nodes[pr.pair] = nodes;
            out.fail_group[pr.pair] = fail;
            out.pods[pr.pair] = placed;
            out.new_pods[pr.pair] = on_new;
            if (nodes >= 0) atomicMin(&out.best[pr.job], (unsigned long long)nodes << 32 | (uint32_t)pr.pair);
          }
        }
      });
}

}  // namespace

hipError_t launch_scale(hipStream_t s, const ScaleIn& in, int64_t blocks, const FitLarge* large, int64_t* scratch,
                        const PlaceSegs& segs, const ScaleOut& out) {
  if (blocks <= 0) return hipSuccess;
  if (blocks > (int64_t)INT32_MAX || in.n_new < 0 || in.n_new > SCALE_MAX_NODES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(large ? scale_domains_kernel<false> : scale_domains_kernel<true>, dim3((unsigned)blocks),
                     dim3(PL_THREADS), 0, s, in, large, scratch, (const int32_t*)segs.seg_off, (const uint32_t*)segs.gid,
                     (const uint32_t*)segs.lab, (const int64_t*)segs.res, segs.seg_stride, out);
  return hipGetLastError();
}

}  // namespace pe
