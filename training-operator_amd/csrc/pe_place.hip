// Gang placement inside a chosen topology domain (pe_place_greedy_domains).  Jobs pinned to different
// domains touch disjoint nodes, so the sequential greedy rule binds only inside a
// domain: one workgroup per ACTIVE domain (a domain with at least one job) runs its jobs' decisions on the
// device, all domains in parallel -- no host resolver, no windows, no candidate lists.
//
// Member lists (place_count_kernel, place_scan_kernel, place_fill_kernel): every node's level-`level` domain
// through the plan's leaf_dom, its active index through act_of; the nodes are counted per active domain, the
// counts scanned into segment bounds, and each node's state (global id, labels, four residuals) is gathered
// into its domain's segment, so the placement reads contiguous memory.  A node's place inside its segment
// comes from an atomic cursor and differs from run to run; every key carries the node id (unique, low 24
// bits), so no result depends on that order.  A domain without nodes has a zero-length segment and still
// gets its workgroup, which fails the jobs that have pods and passes the others.
//
// place_domains_kernel: the workgroup walks its jobs in plan order, group by group.  The decision and the walk
// of a job's groups through it are pe_place_step.h's, shared with every other domain call; the log, the pod
// stores, the rollback (place_job) and the stage / run / write-back frame of the kernel (place_frame) are
// pe_place_job.h's, shared with pe_place_min.hip; this file owns the member lists, a domain's loop over its
// jobs and the first-fit rounds.  Per decision every
// thread scores its share of the segment with node_key (pe_node_key.h) against the working residuals and
// finds what its own best node would take; a wave butterfly (pe_wave.h) and one cross-wave step through LDS
// give the block's minimum key with that node's place and take.  The chosen node takes
//   t = min(pods left, min over d with q_d > 0 of floor(res_d / q_d))      (no q_d > 0: all the pods left)
// pods at once -- exact: a node's key never rises as its leftover falls, so it stays the minimum while it
// fits (the host resolver does the same), and counts reach 2^31 - 1, so one pod per
// decision is not an option.  An island group is one decision for count x request.  Thread i mod PL_THREADS
// is the only one that reads or writes place i of the working state outside a rollback, so a decision costs
// one barrier.  A job that cannot place a pod gives back what it took from its log of (place, group, pods)
// entries -- kept in the job's own pod range of the scratch array: every entry places at least one pod --
// and its pod slots become -1.  The working state lives in LDS for segments up to PL_LDS_NODES nodes and in
// the global segment beyond (two instances of the kernel, each taking its kind of segment); at the end the
// workgroup writes its nodes' residuals back to the live SoA.
//
// first_fit_round_kernel (pe_place_first_fit_domains): the same decisions job by job (place_job, pe_place_job.h), with every job
// free to move on to its next candidate domain; the comment at first_fit_queue has the scheme.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_place_step.h"

namespace pe {

namespace {

constexpr int PM_THREADS = 256;

// The active index of local node n, -1 for none.
__device__ __forceinline__ int node_active(const int32_t* __restrict__ island, int64_t n,
                                           const int32_t* __restrict__ leaf_dom, int n_leaf,
                                           const int32_t* __restrict__ act_of) {
  const int32_t isl = island[n];
  if ((uint32_t)isl >= (uint32_t)n_leaf) return -1;
  const int32_t d = leaf_dom[isl];   // < the level's size: the plan validated the map
  return d < 0 ? -1 : act_of[d];
}

// ctr[a] += 1 for every lane with a >= 0; returns the lane's value before (unspecified for a < 0).  A wave
// whose lanes all name one domain -- contiguous racks -- issues one atomic instead of 64.  Called by whole waves.
__device__ __forceinline__ int32_t wave_take(int a, int32_t* ctr, int lane) {
  const int first = __builtin_amdgcn_readfirstlane(a);
  if (__all(a == first)) {
    if (first < 0) return 0;
    int32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctr[first], 64);
    return __builtin_amdgcn_readfirstlane(base) + lane;
  }
  return a >= 0 ? atomicAdd(&ctr[a], 1) : 0;
}

__global__ __launch_bounds__(PM_THREADS) void place_count_kernel(const int32_t* __restrict__ island, int64_t Ns,
                                                                 const int32_t* __restrict__ leaf_dom, int n_leaf,
                                                                 const int32_t* __restrict__ act_of,
                                                                 int32_t* __restrict__ cnt) {
  const int64_t n = (int64_t)blockIdx.x * PM_THREADS + threadIdx.x;
  const int a = n < Ns ? node_active(island, n, leaf_dom, n_leaf, act_of) : -1;
  (void)wave_take(a, cnt, threadIdx.x & 63);
}

// seg_off[0 .. A] = exclusive scan of cnt[0 .. A), cursor[a] = seg_off[a].  One block: A <= 65536.
__global__ __launch_bounds__(1024) void place_scan_kernel(const int32_t* __restrict__ cnt, int A,
                                                          int32_t* __restrict__ seg_off, int32_t* __restrict__ cursor) {
  __shared__ int32_t part[1024];
  const int tid = threadIdx.x;
  const int per = (A + 1023) / 1024;
  const int lo = min(tid * per, A), hi = min(lo + per, A);
  int32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int32_t v = part[i];
      part[i] = run;
      run += v;
    }
    seg_off[A] = run;
  }
  __syncthreads();
  int32_t run = part[tid];
  for (int i = lo; i < hi; ++i) {
    seg_off[i] = run;
    cursor[i] = run;
    run += cnt[i];
  }
}

__global__ __launch_bounds__(PM_THREADS) void place_fill_kernel(
    const int64_t* __restrict__ res, int64_t stride, const uint32_t* __restrict__ labels,
    const int32_t* __restrict__ island, int64_t Ns, uint32_t id_base, const int32_t* __restrict__ leaf_dom, int n_leaf,
    const int32_t* __restrict__ act_of, PlaceSegs sg) {
  const int64_t n = (int64_t)blockIdx.x * PM_THREADS + threadIdx.x;
  const int a = n < Ns ? node_active(island, n, leaf_dom, n_leaf, act_of) : -1;
  const int32_t at = wave_take(a, sg.cursor, threadIdx.x & 63);   // < seg_off[a + 1] <= Ns: the count pass saw the same nodes
  if (a < 0) return;
  sg.gid[at] = id_base + (uint32_t)n;
  sg.lab[at] = labels[n];
#pragma unroll
  for (int d = 0; d < D; ++d) sg.res[d * sg.seg_stride + at] = res[d * stride + n];
}

// One domain's jobs jobs[j0 .. j1), in that order, on its n nodes (the working state as for place_job).
template <class Stride>
__device__ __forceinline__ void place_domain(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn,
                                             const PlaceGroup* __restrict__ groups, const PlaceJob* __restrict__ jobs,
                                             int j0, int j1, int32_t* __restrict__ out_pod,
                                             int32_t* __restrict__ out_status, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  int par = 0;
  for (int ji = j0; ji < j1; ++ji) {
    const int g0 = jobs[ji].g0, g1 = jobs[ji].g1;
    if (g0 == g1) {   // no groups: placed
      if (tid == 0) out_status[jobs[ji].job] = 0;
      continue;
    }
    const bool ok = place_job(r0, gid, rs, n, mn, par, groups, g0, g1, out_pod, log);
    if (tid == 0) out_status[jobs[ji].job] = ok ? 0 : 1;
  }
}

// place_frame (pe_place_job.h) around place_domain.  IN_LDS: the instance for the segments of at most
// PL_LDS_NODES nodes, whose working state it stages in LDS; the other instance takes the larger segments and
// works on the global segment in place.  Both are launched over all the active domains and a workgroup whose
// segment is the other instance's leaves at once (one kernel with both paths held more uniform values than
// there are SGPRs).
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void place_domains_kernel(
    const PlaceGroup* __restrict__ groups, const PlaceJob* __restrict__ jobs, const int32_t* __restrict__ job_start,
    PlaceSegs sg, int64_t* __restrict__ res, int64_t stride, uint32_t id_base, int32_t* __restrict__ out_pod,
    int32_t* __restrict__ out_status, int32_t* __restrict__ log) {
  place_frame<IN_LDS>(sg, res, stride, id_base, [&](int64_t* r0, const uint32_t* gid, auto rs, int n, PlaceMin& mn) {
    const int a = blockIdx.x;
    place_domain(r0, gid, rs, n, mn, groups, jobs, job_start[a], job_start[a + 1], out_pod, out_status, log);
  });
}

// ---- pe_place_first_fit_domains: one round.  The workgroup of active domain a looks at the head of its queue.
// Whatever it reads of another job's word it reads as the word stood when the round began: a word stamped with
// this round was written by an attempt at position k' of this very round (a job is attempted at most once per
// round: its stamped word stops every other entry of it), so the value before was k', unsettled.  An entry whose
// job has moved past it is skipped, an entry whose job is due here is attempted -- place_job's decisions and
// rollback -- and an entry whose job is still busy elsewhere ends the round for this domain.  Nothing depends on
// which workgroup ran first, nobody waits for anybody, and pods, residuals and logs pass from workgroup to
// workgroup only across the kernel boundary.  The head of the queue has the lowest rank among the entries still
// open at this domain, so an attempt sees the domain as the sequential rule leaves it.
template <class Stride, class Stage>
__device__ __forceinline__ bool first_fit_queue(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn,
                                                uint64_t* head, const PlaceGroup* __restrict__ groups,
                                                const PlaceJob* __restrict__ jobs,
                                                const FirstFitEntry* __restrict__ queue, int cur, int end, int a,
                                                uint32_t round, const FirstFitState& st, int32_t* __restrict__ out_pod,
                                                int32_t* __restrict__ out_status, int32_t* __restrict__ out_pair,
                                                int32_t* __restrict__ log, Stage stage) {
  const int tid = threadIdx.x;
  int par = 0, hp = 0;
  bool staged = false;
  for (; cur < end; ++cur) {
    const FirstFitEntry e = queue[cur];
    if (tid == 0) head[hp] = __hip_atomic_load(&st.word[e.job], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();   // head[] is used in turn, as PlaceMin's sets are: one barrier per entry
    const uint64_t w = head[hp];
    hp ^= 1;
    const uint32_t stamp = (uint32_t)(w >> 32);
    uint32_t ptr = (uint32_t)w;
    if (stamp == round) ptr = (ptr & FF_SETTLED) ? (ptr & ~FF_SETTLED) : ptr - 1;   // as the round began
    if ((ptr & FF_SETTLED) || ptr > (uint32_t)e.k) continue;   // settled, or past this candidate
    if (ptr < (uint32_t)e.k || stamp == round) break;          // busy elsewhere: the next round's
    if (!staged) {
      stage();
      staged = true;
    }
    const PlaceJob pj = jobs[e.job];
    const bool ok = pj.g0 == pj.g1 || place_job(r0, gid, rs, n, mn, par, groups, pj.g0, pj.g1, out_pod, log);
    if (tid == 0) {
      uint32_t next = (uint32_t)e.k + 1;
      if (ok) {
        out_status[e.job] = 0;
        out_pair[e.job] = e.pair;
      }
      if (ok || e.last) {
        next = FF_SETTLED | (uint32_t)e.k;
        atomicSub(st.open, 1u);
      }
      __hip_atomic_store(&st.word[e.job], ((uint64_t)round << 32) | next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid == 0) st.cursor[a] = cur;
  return staged;
}

// IN_LDS as for place_domains_kernel: the segments of at most PL_LDS_NODES nodes are staged in LDS before the
// round's first attempt and written back to the segment after its last; the larger ones are worked on in place.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void first_fit_round_kernel(
    const PlaceGroup* __restrict__ groups, const PlaceJob* __restrict__ jobs, const int32_t* __restrict__ q_start,
    const FirstFitEntry* __restrict__ queue, PlaceSegs sg, uint32_t round, FirstFitState st,
    int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status, int32_t* __restrict__ out_pair,
    int32_t* __restrict__ log) {
  __shared__ PlaceMin mn;
  __shared__ uint64_t head[2];
  const int a = blockIdx.x, tid = threadIdx.x;
  const int cur = st.cursor[a], end = q_start[a + 1];   // the cursor is this workgroup's own, round after round
  if (cur >= end) return;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= PL_LDS_NODES) != IN_LDS) return;
  int64_t* const g0 = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  if constexpr (IN_LDS) {
    __shared__ PlaceShared sh;
    const bool staged = first_fit_queue(
        sh.r[0], sh.gid, std::integral_constant<int, PL_LDS_NODES>(), n, mn, head, groups, jobs, queue, cur, end, a, round,
        st, out_pod, out_status, out_pair, log, [&]() {
          for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
#pragma unroll
            for (int d = 0; d < D; ++d) sh.r[d][i] = g0[d * ss + i];
            sh.lab[i] = gid[ss + i];
            sh.gid[i] = gid[i];
          }
        });
    if (staged)
      for (int i = tid; i < n; i += PL_THREADS) {
#pragma unroll
        for (int d = 0; d < D; ++d) g0[d * ss + i] = sh.r[d][i];
      }
  } else {
    (void)first_fit_queue(g0, gid, ss, n, mn, head, groups, jobs, queue, cur, end, a, round, st, out_pod, out_status,
                          out_pair, log, []() {});
  }
}

__global__ __launch_bounds__(PM_THREADS) void first_fit_finish_kernel(PlaceSegs sg, int A, int64_t* __restrict__ res,
                                                                     int64_t stride, uint32_t id_base) {
  const int64_t i = (int64_t)blockIdx.x * PM_THREADS + threadIdx.x;
  if (i >= sg.seg_off[A]) return;   // <= Ns places, every node in at most one segment
  const int64_t l = (int64_t)(sg.gid[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
  for (int d = 0; d < D; ++d) res[d * stride + l] = sg.res[d * sg.seg_stride + i];
}

}  // namespace

hipError_t launch_place_members(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                const int32_t* island, int64_t Ns, uint64_t id_base, const int32_t* leaf_dom,
                                int n_leaf, const int32_t* act_of, int A, const PlaceSegs& segs) {
  if (A <= 0 || A > DM_MAX_DOMAINS || Ns < 0 || Ns > (int64_t(1) << 24)) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((Ns + PM_THREADS - 1) / PM_THREADS);
  if (blocks > 0)
    hipLaunchKernelGGL(place_count_kernel, dim3(blocks), dim3(PM_THREADS), 0, s, island, Ns, leaf_dom, n_leaf, act_of,
                       segs.cnt);
  hipLaunchKernelGGL(place_scan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t*)segs.cnt, A, segs.seg_off,
                     segs.cursor);
  if (blocks > 0)
    hipLaunchKernelGGL(place_fill_kernel, dim3(blocks), dim3(PM_THREADS), 0, s, res, stride, labels, island, Ns,
                       (uint32_t)id_base, leaf_dom, n_leaf, act_of, segs);
  return hipGetLastError();
}

hipError_t launch_place_domains(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* job_start,
                                int A, const PlaceSegs& segs, int64_t* res, int64_t stride, uint64_t id_base,
                                int32_t* out_pod, int32_t* out_status, int32_t* log) {
  if (A <= 0) return hipSuccess;
  hipLaunchKernelGGL(place_domains_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     res, stride, (uint32_t)id_base, out_pod, out_status, log);
  hipLaunchKernelGGL(place_domains_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     res, stride, (uint32_t)id_base, out_pod, out_status, log);
  return hipGetLastError();
}

hipError_t launch_first_fit_round(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* q_start,
                                  const FirstFitEntry* queue, int A, const PlaceSegs& segs, int kinds, uint32_t round,
                                  const FirstFitState& st, int32_t* out_pod, int32_t* out_status, int32_t* out_pair,
                                  int32_t* log) {
  if (A <= 0) return hipSuccess;
  if (round == 0) return hipErrorInvalidValue;   // the zeroed words carry stamp 0
  if (kinds & FF_SMALL)
    hipLaunchKernelGGL(first_fit_round_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, q_start,
                       queue, segs, round, st, out_pod, out_status, out_pair, log);
  if (kinds & FF_LARGE)
    hipLaunchKernelGGL(first_fit_round_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, q_start,
                       queue, segs, round, st, out_pod, out_status, out_pair, log);
  return hipGetLastError();
}

hipError_t launch_first_fit_finish(hipStream_t s, const PlaceSegs& segs, int A, int64_t Ns, int64_t* res, int64_t stride,
                                   uint64_t id_base) {
  const unsigned blocks = (unsigned)((Ns + PM_THREADS - 1) / PM_THREADS);
  if (A <= 0 || blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(first_fit_finish_kernel, dim3(blocks), dim3(PM_THREADS), 0, s, segs, A, res, stride, (uint32_t)id_base);
  return hipGetLastError();
}

}  // namespace pe
