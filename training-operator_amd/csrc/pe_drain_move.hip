// Drain a batch of nodes, moving as it goes (pe_drain_move_domains): pe_drain_fit_domains' question asked of a LIST
// of nodes that are cordoned together and emptied one after the other.  The placing frame of pe_place.hip -- one
// workgroup per active target domain, the working state in LDS for segments of at most PL_LDS_NODES nodes and the
// compact global segment beyond -- around the drain plan's runs (pe_drain_plan.h).
//
// ONE EVOLVING STATE.  drain_domains_kernel (pe_drain.hip) judges every candidate alone, so each judgement starts
// from a fresh copy of the segment without the candidate's node.  Here a domain's candidates are a sequence: the
// segment is staged ONCE, the takes of a candidate that fits stay in it, and a candidate that fails gives back
// exactly what its log says (place_rollback: two's-complement adds cancel bit for bit).  No copy is made per
// candidate; a candidate costs its decisions and, where it fails, one pass over its log.
//
// THE CORDON.  Every candidate node of the call is out of every decision of the call.  drain_cordon_kernel sets one
// bit per candidate in a bitmap over the node ids (vector atomics: 32 nodes share a word).  The staging pass tests
// gid[i] against it and writes NEVER into all four rows of a cordoned place -- what a removed slot holds, so that no
// request, not even a zero one, fits it.  The thread that stages place i is the only one that scores it, so the
// cordon costs no barrier.  place_frame's write-back would store those NEVERs into the live SoA; this file's frame
// tests the same bit again and leaves cordoned places alone.  They are then exactly the places
// drain_move_sweep_kernel may add to, whatever segment they lie in: a candidate whose node is a member of ANOTHER
// active target domain is skipped by that domain's workgroup too.
//
// A candidate's pods and log live in its own range of the slot list: moved[E] is parallel to slot_list[E] (place
// p of the list moved to node moved[p], -1 = not moved) and the log is place_job's, 3 int32 per entry at
// log[3 (first place + entry)] -- an entry places at least one pod, so the candidate's range holds it.
//
// drain_move_sweep_kernel, a launch of its own behind both instances: it strides over the E places, scatters
// target[slot_list[p]] = moved[p] and -- unless the call is a dry run -- gives every evicted pod of a candidate that
// fits back to the candidate's node in the live SoA.  Many places name one node: atomic adds.  No decision read
// those cells, and no workgroup wrote them.
//
// Integer code throughout, plain C++ and vector stores only.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_place_step.h"

namespace pe {

namespace {

__device__ __forceinline__ bool cordoned(const uint32_t* __restrict__ cordon, uint32_t id) {
  return (cordon[id >> 5] >> (id & 31)) & 1u;
}

constexpr int DC_THREADS = 256;

// One bit per candidate node.  nodes of pairs[0 .. C) lie in [0, n_total): the plan validated them.
__global__ __launch_bounds__(DC_THREADS) void drain_cordon_kernel(const DrainPair* __restrict__ pairs, int64_t C,
                                                                  uint32_t* __restrict__ cordon) {
  const int64_t i = (int64_t)blockIdx.x * DC_THREADS + threadIdx.x;
  if (i >= C) return;
  const uint32_t id = (uint32_t)pairs[i].node;
  atomicOr(&cordon[id >> 5], 1u << (id & 31));
}

// One domain's candidates pairs[p0 .. p1), in that order, on its n nodes (the working state as for place_job).
// The walk is place_job's with the failing run and the pods placed so far handed out: the call answers where the
// rule stopped.
template <class Stride>
__device__ __forceinline__ void drain_move_domain(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn,
                                                  const DrainMoveIn& in, int p0, int p1, const DrainOut& out,
                                                  int32_t* __restrict__ moved_row, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  const PlaceGroup* const runs = in.runs;
  int par = 0;
  for (int pi = p0; pi < p1; ++pi) {
    const DrainPair pr = in.pairs[pi];
    int64_t moved = 0, fail_at = -1;
    if (pr.g0 < pr.g1) {   // a candidate without pods fits as it is
      const int64_t c0 = runs[pr.g0].pod0;   // its places of the slot list: [c0, c1)
      int64_t n_log = 0;
      uint32_t left;
      const int g = place_groups(r0, rs, gid, gid + rs, n, mn, par, runs, pr.g0, pr.g1, left,
                                 [&](int gi, const PlaceGroup& gr, const PlaceChoice& c, uint32_t done) {
                                   if (tid == 0) {   // n_log < the pods placed so far, this decision's included
                                     int32_t* const e = log + 3 * (c0 + n_log);
                                     e[0] = (int32_t)c.at;
                                     e[1] = gi;
                                     e[2] = (int32_t)c.t;
                                   }
                                   ++n_log;
                                   const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
                                   const int64_t at = gr.pod0 + done;   // at + t <= c1 <= E
                                   for (int64_t p = at + tid; p < at + c.t; p += PL_THREADS) moved_row[p] = node;
                                   moved += c.t;
                                 });
      if (g < pr.g1) {
        // the place of the first pod that found no node: an island run fails as a whole, with all its pods left
        fail_at = runs[g].pod0 + (int64_t)((uint32_t)runs[g].count - left);
        const int64_t c1 = runs[pr.g1 - 1].pod0 + runs[pr.g1 - 1].count;
        __syncthreads();   // the log's last entry, the last take and the last pod store are written
        place_rollback(r0, (int64_t)rs, runs, log + 3 * c0, n_log, moved_row + c0, c1 - c0);
        __syncthreads();   // the owners read their places again
      }
    }
    if (tid == 0) {   // pr.cand < C: the plan validated the list
      out.fits[pr.cand] = fail_at < 0;
      out.moved[pr.cand] = moved;
      out.fail_slot[pr.cand] = fail_at < 0 ? -1 : (int64_t)in.slot_list[fail_at];
    }
  }
}

// The frame: stage with the cordon, run the domain's candidates, write back what is not cordoned (nothing in a dry
// run).  IN_LDS as for place_domains_kernel: two instances, each taking its kind of segment.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void drain_move_kernel(DrainMoveIn in, PlaceSegs sg, int64_t* __restrict__ res,
                                                                int64_t stride, uint32_t id_base, int dry_run,
                                                                DrainOut out, int32_t* __restrict__ moved_row,
                                                                int32_t* __restrict__ log) {
  __shared__ PlaceMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= PL_LDS_NODES) != IN_LDS) return;
  int64_t* const g0 = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  const int p0 = in.pair_start[a], p1 = in.pair_start[a + 1];
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs) {
    drain_move_domain(r0, ids, rs, n, mn, in, p0, p1, out, moved_row, log);
    if (dry_run) return;
    for (int i = tid; i < n; i += PL_THREADS) {   // place i is its owner's, and the last barrier is behind
      if (cordoned(in.cordon, ids[i])) continue;   // the sweep's cells
      const int64_t l = (int64_t)(ids[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
      for (int d = 0; d < D; ++d) res[d * stride + l] = r0[d * rs + i];
    }
  };
  if constexpr (IN_LDS) {
    __shared__ PlaceShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
      const uint32_t id = gid[i];
      const bool off = cordoned(in.cordon, id);
#pragma unroll
      for (int d = 0; d < D; ++d) sh.r[d][i] = off ? NEVER : g0[d * ss + i];
      sh.lab[i] = gid[ss + i];
      sh.gid[i] = id;
    }
    run(sh.r[0], sh.gid, std::integral_constant<int, PL_LDS_NODES>());
  } else {
    for (int i = tid; i < n; i += PL_THREADS) {   // the compact segment is the call's own copy
      if (!cordoned(in.cordon, gid[i])) continue;
#pragma unroll
      for (int d = 0; d < D; ++d) g0[d * ss + i] = NEVER;
    }
    run(g0, gid, ss);
  }
}

constexpr int SW_THREADS = 256, SW_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(SW_THREADS) void drain_move_sweep_kernel(DrainMoveIn in, int64_t E,
                                                                      const uint8_t* __restrict__ fits,
                                                                      const int32_t* __restrict__ moved_row,
                                                                      int32_t* __restrict__ target,
                                                                      int64_t* __restrict__ res, int64_t stride,
                                                                      uint32_t id_base, int dry_run) {
  for (int64_t p = (int64_t)blockIdx.x * SW_THREADS + threadIdx.x; p < E; p += (int64_t)gridDim.x * SW_THREADS) {
    if (target) target[in.slot_list[p]] = moved_row[p];   // every slot < S: the plan's list
    if (dry_run) continue;
    const int r = in.run_of[p];
    const DrainPair pr = in.pairs[in.run_pair[r]];
    if (!fits[pr.cand]) continue;
    const int64_t l = (int64_t)((uint32_t)pr.node - id_base);   // < Ns; live: a removed candidate evicts nothing
#pragma unroll
    for (int d = 0; d < D; ++d) {   // many places name one node
      const int64_t q = in.runs[r].q[d];
      if (q != 0) atomicAdd((unsigned long long*)&res[d * stride + l], (unsigned long long)q);
    }
  }
}

}  // namespace

hipError_t launch_drain_cordon(hipStream_t s, const DrainPair* pairs, int64_t C, uint32_t* cordon) {
  if (C <= 0) return hipSuccess;
  hipLaunchKernelGGL(drain_cordon_kernel, dim3((unsigned)((C + DC_THREADS - 1) / DC_THREADS)), dim3(DC_THREADS), 0, s,
                     pairs, C, cordon);
  return hipGetLastError();
}

hipError_t launch_drain_move(hipStream_t s, const DrainMoveIn& in, int A, const PlaceSegs& segs, int64_t* res,
                             int64_t stride, uint32_t id_base, bool dry_run, const DrainOut& out, int32_t* moved_row,
                             int32_t* log) {
  if (A <= 0) return hipSuccess;
  hipLaunchKernelGGL(drain_move_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, in, segs, res, stride, id_base,
                     (int)dry_run, out, moved_row, log);
  hipLaunchKernelGGL(drain_move_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, in, segs, res, stride, id_base,
                     (int)dry_run, out, moved_row, log);
  return hipGetLastError();
}

hipError_t launch_drain_move_sweep(hipStream_t s, const DrainMoveIn& in, int64_t E, const uint8_t* fits,
                                   const int32_t* moved_row, int32_t* target, int64_t* res, int64_t stride,
                                   uint32_t id_base, bool dry_run) {
  if (E <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((E + SW_THREADS - 1) / SW_THREADS, SW_MAX_BLOCKS);
  hipLaunchKernelGGL(drain_move_sweep_kernel, dim3((unsigned)blocks), dim3(SW_THREADS), 0, s, in, E, fits, moved_row,
                     target, res, stride, id_base, (int)dry_run);
  return hipGetLastError();
}

}  // namespace pe
