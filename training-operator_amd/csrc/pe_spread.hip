// Gang placement with per-domain pod caps (pe_place_spread_domains): pe_place.hip's scheme -- one workgroup per
// active domain, its jobs in plan order on the domain's compact segment -- with pe_spread_step.h's decision, which
// knows a cap: a group with cap m puts at most m of its pods into one spread domain, the node itself or the node's
// domain at a level below the placing level (podAntiAffinity / topologySpreadConstraints on hostname or on a rack
// key).  The take-many argument under the cap and the lazy allowance are stated in pe_spread_step.h.
//
// spread_sub_kernel: every place of every segment learns which spread domain of its segment it is in, from the
// plan's leaf_sub through the node's leaf; only for spread domains above the node.
//
// spread_domains_kernel<IN_LDS, BY_NODE>: four instances.  The working state of a place is pe_place.hip's 40 B
// (four residuals, labels, id) and 4 B of allowance, with 4 B of `sub` more when the spread domain is not the node
// -- so each kind has its own instance and its own LDS limit, the largest segment that keeps the workgroup within
// the 40 KiB at which four of them share a CU (pe_kernels.h: SP_LDS_NODES_NODE, SP_LDS_NODES_DOM).  A larger segment
// is worked on in place on the compact global segment, with the allowance row (and the sub row, which every
// instance of the second kind reads) in the call's scratch.  The job frame is place_job's: a log of (place, group,
// pods) per take in the job's own pod range, pod stores by the whole block, place_rollback for a failed job.  The
// allowances are per group and rebuilt at each group start, so a rollback does not touch them.  A dry run skips
// the write-back to the live residuals and nothing else: the segment is a copy, so later jobs of a domain still
// see earlier jobs' takes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_spread_step.h"

namespace pe {

namespace {

constexpr int SS_THREADS = 256;

// sub[i] = leaf_sub[the leaf of place i's node] for the places [0, seg_off[A]) of all segments.
__global__ __launch_bounds__(SS_THREADS) void spread_sub_kernel(PlaceSegs sg, int A, const int32_t* __restrict__ island,
                                                                uint32_t id_base, const int32_t* __restrict__ leaf_sub,
                                                                uint32_t* __restrict__ sub) {
  const int64_t i = (int64_t)blockIdx.x * SS_THREADS + threadIdx.x;
  if (i >= sg.seg_off[A]) return;   // <= Ns places, every node in at most one segment
  const int64_t l = (int64_t)(sg.gid[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
  sub[i] = (uint32_t)leaf_sub[island[l]];   // a node of a segment has a leaf in [0, n_leaf): the fill kernel's test
}

template <bool BY_NODE>
struct SpreadShared;
template <>
struct SpreadShared<true> {
  static constexpr int N = SP_LDS_NODES_NODE;
  int64_t r[D][N];
  uint32_t gid[N], lab[N], allow[N];
  __device__ __forceinline__ uint32_t* sub_row() { return nullptr; }
};
template <>
struct SpreadShared<false> {
  static constexpr int N = SP_LDS_NODES_DOM;
  int64_t r[D][N];
  uint32_t gid[N], lab[N], allow[N], sub[N];
  __device__ __forceinline__ uint32_t* sub_row() { return sub; }
};
static_assert(sizeof(SpreadShared<true>) + sizeof(PlaceMin) <= 40 * 1024 &&
                  sizeof(SpreadShared<true>) + sizeof(PlaceMin) + 44 > 40 * 1024,
              "SP_LDS_NODES_NODE: the largest segment within 40 KiB");
static_assert(sizeof(SpreadShared<false>) + sizeof(PlaceMin) <= 40 * 1024 &&
                  sizeof(SpreadShared<false>) + sizeof(PlaceMin) + 48 > 40 * 1024,
              "SP_LDS_NODES_DOM: the largest segment within 40 KiB");

// place_job with the groups' caps: one job (groups [g0, g1), g0 < g1) on a domain's n nodes, all or nothing.
template <bool BY_NODE, class Stride>
__device__ __forceinline__ bool spread_job(int64_t* r0, const uint32_t* gid, Stride rs, uint32_t* allow,
                                           const uint32_t* sub, int n, PlaceMin& mn, int& par,
                                           const PlaceGroup* __restrict__ groups, const int32_t* __restrict__ caps, int g0,
                                           int g1, int32_t* __restrict__ out_pod, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  const int64_t pod0 = groups[g0].pod0;   // the job's pod slots: [pod0, the last group's pod0 + count)
  int64_t n_log = 0;                      // entries of this job, at log[3 pod0 ..]; <= the pods it placed
  uint32_t left;
  const bool ok =
      spread_groups<BY_NODE>(r0, rs, gid, gid + rs, allow, sub, n, mn, par, groups, caps, g0, g1, left,
                             [&](int g, const PlaceGroup& gr, const PlaceChoice& c, uint32_t done) {
                               if (tid == 0) {
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
    __syncthreads();   // every update and pod store of this job lies before the decision that failed
    place_rollback(r0, (int64_t)rs, groups, log + 3 * pod0, n_log, out_pod + pod0,
                   groups[g1 - 1].pod0 + groups[g1 - 1].count - pod0);
    __syncthreads();   // the owners read their places again
  }
  return ok;
}

// One workgroup per active domain a = blockIdx.x; a workgroup whose segment is the other instance's leaves at once.
// allow_row / sub_row: the call's scratch rows, parallel to the segments' places (sub_row: !BY_NODE only).
template <bool IN_LDS, bool BY_NODE>
__global__ __launch_bounds__(PL_THREADS) void spread_domains_kernel(
    const PlaceGroup* __restrict__ groups, const int32_t* __restrict__ caps, const PlaceJob* __restrict__ jobs,
    const int32_t* __restrict__ job_start, PlaceSegs sg, uint32_t* __restrict__ allow_row,
    const uint32_t* __restrict__ sub_row, int64_t* __restrict__ res, int64_t stride, uint32_t id_base, int dry_run,
    int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status, int32_t* __restrict__ log) {
  using Shared = SpreadShared<BY_NODE>;
  __shared__ PlaceMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= Shared::N) != IN_LDS) return;
  int64_t* const seg = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs, uint32_t* allow, const uint32_t* sub) {
    int par = 0;
    for (int ji = job_start[a]; ji < job_start[a + 1]; ++ji) {
      const PlaceJob pj = jobs[ji];
      const bool ok = pj.g0 == pj.g1 ||   // no groups: placed
                      spread_job<BY_NODE>(r0, ids, rs, allow, sub, n, mn, par, groups, caps, pj.g0, pj.g1, out_pod, log);
      if (tid == 0) out_status[pj.job] = ok ? 0 : 1;
    }
    if (dry_run) return;
    for (int i = tid; i < n; i += PL_THREADS) {
      const int64_t l = (int64_t)(ids[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
      for (int d = 0; d < D; ++d) res[d * stride + l] = r0[d * rs + i];
    }
  };
  if constexpr (IN_LDS) {
    __shared__ Shared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
#pragma unroll
      for (int d = 0; d < D; ++d) sh.r[d][i] = seg[d * ss + i];
      sh.lab[i] = gid[ss + i];
      sh.gid[i] = gid[i];
      if constexpr (!BY_NODE) sh.sub[i] = sub_row[b + i];
    }
    run(sh.r[0], sh.gid, std::integral_constant<int, Shared::N>(), sh.allow, sh.sub_row());
  } else {
    run(seg, gid, ss, allow_row + b, BY_NODE ? nullptr : sub_row + b);
  }
}

template <bool IN_LDS, bool BY_NODE>
void launch_instance(hipStream_t s, const PlaceGroup* groups, const int32_t* caps, const PlaceJob* jobs,
                     const int32_t* job_start, int A, const PlaceSegs& segs, uint32_t* allow_row, const uint32_t* sub_row,
                     int64_t* res, int64_t stride, uint64_t id_base, bool dry_run, int32_t* out_pod, int32_t* out_status,
                     int32_t* log) {
  hipLaunchKernelGGL((spread_domains_kernel<IN_LDS, BY_NODE>), dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, caps,
                     jobs, job_start, segs, allow_row, sub_row, res, stride, (uint32_t)id_base, dry_run ? 1 : 0, out_pod,
                     out_status, log);
}

}  // namespace

hipError_t launch_spread_domains(hipStream_t s, const PlaceGroup* groups, const int32_t* caps, const PlaceJob* jobs,
                                 const int32_t* job_start, int A, const PlaceSegs& segs, const int32_t* island, int64_t Ns,
                                 const int32_t* leaf_sub, uint32_t* allow_row, uint32_t* sub_row, int64_t* res,
                                 int64_t stride, uint64_t id_base, bool dry_run, int32_t* out_pod, int32_t* out_status,
                                 int32_t* log) {
  if (A <= 0) return hipSuccess;
  if (A > DM_MAX_DOMAINS || Ns < 0 || Ns > (int64_t(1) << 24) || !allow_row) return hipErrorInvalidValue;
  const bool by_node = leaf_sub == nullptr;
  if (!by_node) {
    if (!sub_row || !island) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((Ns + SS_THREADS - 1) / SS_THREADS);
    if (blocks > 0)
      hipLaunchKernelGGL(spread_sub_kernel, dim3(blocks), dim3(SS_THREADS), 0, s, segs, A, island, (uint32_t)id_base,
                         leaf_sub, sub_row);
    launch_instance<true, false>(s, groups, caps, jobs, job_start, A, segs, allow_row, sub_row, res, stride, id_base,
                                 dry_run, out_pod, out_status, log);
    launch_instance<false, false>(s, groups, caps, jobs, job_start, A, segs, allow_row, sub_row, res, stride, id_base,
                                  dry_run, out_pod, out_status, log);
  } else {
    launch_instance<true, true>(s, groups, caps, jobs, job_start, A, segs, allow_row, nullptr, res, stride, id_base,
                                dry_run, out_pod, out_status, log);
    launch_instance<false, true>(s, groups, caps, jobs, job_start, A, segs, allow_row, nullptr, res, stride, id_base,
                                 dry_run, out_pod, out_status, log);
  }
  return hipGetLastError();
}

}  // namespace pe
