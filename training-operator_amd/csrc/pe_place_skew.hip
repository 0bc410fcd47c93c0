// Gang placement under maxSkew spread (pe_place_skew_domains): pe_place.hip's scheme -- one workgroup per active
// domain, its jobs in plan order on the domain's compact segment -- with pe_skew_step.h's decision, which knows
// topologySpreadConstraints' maxSkew with whenUnsatisfiable: DoNotSchedule.  Why a cap's decision does not do, the
// uniform skew state and the take-many argument are stated in pe_skew_step.h.
//
// skew_clear_kernel, skew_first_kernel, skew_sub_kernel: the key -> place row and the places' `sub`.  The key of a
// place is its spread domain -- the node (its local id) or the node's domain at the spread level, through the plan's
// leaf_sd -- and where[key] is the key's FIRST place among all segments, an atomic minimum over the places.  sub[i] =
// where[key(i)]: the representative of place i's spread domain, in the same segment, since a spread domain lies inside
// one domain of the placing level.  The same row takes a book entry to its place at a group's start, so the node kind
// needs no inverse row of its own and the domain kind no ranks: a search of the group's list per own place would read
// the list once per place and group, the row is read once per entry.
//
// skew_domains_kernel<IN_LDS>: two instances.  The working state of a place is pe_place.hip's 40 B and two words, sub
// and cnt (48 B), so the instance that stages the segment in LDS has a limit of its own, the largest segment that
// keeps the workgroup within the 40 KiB at which four of them share a CU (pe_kernels.h: SK_LDS_NODES).  A larger
// segment is worked on in place on the compact global segment, with sub and cnt as rows of the call's scratch.  The
// job frame is place_job's: a log of (place, group, pods) per take in the job's own pod range, pod stores by the whole
// block, place_rollback for a failed job.  A dry run skips the write-back to the live residuals and nothing else.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_skew_step.h"

namespace pe {

namespace {

constexpr int SKP_THREADS = 256;

__global__ __launch_bounds__(SKP_THREADS) void skew_clear_kernel(int32_t* __restrict__ where, int64_t n_keys) {
  const int64_t k = (int64_t)blockIdx.x * SKP_THREADS + threadIdx.x;
  if (k < n_keys) where[k] = INT32_MAX;
}

// The key of place i < seg_off[A]: the node's local id (leaf_sd NULL) or the node's spread domain; -1: outside the row.
__device__ __forceinline__ int64_t skew_key(const PlaceSegs& sg, int64_t i, const int32_t* __restrict__ island,
                                            uint32_t id_base, const int32_t* __restrict__ leaf_sd, int64_t n_keys) {
  const int64_t l = (int64_t)(sg.gid[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
  const int64_t k = leaf_sd ? leaf_sd[island[l]] : l;   // a node of a segment has a leaf in [0, n_leaf): the fill kernel's test
  return k >= 0 && k < n_keys ? k : -1;
}

__global__ __launch_bounds__(SKP_THREADS) void skew_first_kernel(PlaceSegs sg, int A, const int32_t* __restrict__ island,
                                                                 uint32_t id_base, const int32_t* __restrict__ leaf_sd,
                                                                 int64_t n_keys, int32_t* __restrict__ where) {
  const int64_t i = (int64_t)blockIdx.x * SKP_THREADS + threadIdx.x;
  if (i >= sg.seg_off[A]) return;   // <= Ns places, every node in at most one segment
  const int64_t k = skew_key(sg, i, island, id_base, leaf_sd, n_keys);
  if (k >= 0) atomicMin(&where[k], (int32_t)i);
}

__global__ __launch_bounds__(SKP_THREADS) void skew_sub_kernel(PlaceSegs sg, int A, const int32_t* __restrict__ island,
                                                               uint32_t id_base, const int32_t* __restrict__ leaf_sd,
                                                               int64_t n_keys, const int32_t* __restrict__ where,
                                                               uint32_t* __restrict__ sub) {
  const int64_t i = (int64_t)blockIdx.x * SKP_THREADS + threadIdx.x;
  if (i >= sg.seg_off[A]) return;
  const int64_t k = skew_key(sg, i, island, id_base, leaf_sd, n_keys);
  sub[i] = k >= 0 ? (uint32_t)where[k] : (uint32_t)i;   // a place without a key stands alone
}

struct SkewShared {
  static constexpr int N = SK_LDS_NODES;
  int64_t r[D][N];
  uint32_t gid[N], lab[N], sub[N], cnt[N];
};
static_assert(sizeof(SkewShared) + sizeof(SkewMin) <= 40 * 1024 && sizeof(SkewShared) + sizeof(SkewMin) + 48 > 40 * 1024,
              "SK_LDS_NODES: the largest segment within 40 KiB");

// place_job with the groups' skews: one job (groups [g0, g1), g0 < g1) on a domain's n nodes, all or nothing.  dec:
// the takes made, carried from job to job.
template <class Stride>
__device__ __forceinline__ bool skew_job(int64_t* r0, const uint32_t* gid, Stride rs, const SkewRows& rw, int n, SkewMin& mn,
                                         int& par, uint32_t& dec, const PlaceGroup* __restrict__ groups, int g0, int g1,
                                         int32_t* __restrict__ out_pod, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  const int64_t pod0 = groups[g0].pod0;   // the job's pod slots: [pod0, the last group's pod0 + count)
  int64_t n_log = 0;                      // entries of this job, at log[3 pod0 ..]; <= the pods it placed
  uint32_t left;
  const bool ok = skew_groups(r0, rs, gid, gid + rs, rw, n, mn, par, groups, g0, g1, left,
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
  dec += (uint32_t)n_log;
  if (!ok) {
    __syncthreads();   // every update and pod store of this job lies before the decision that failed
    place_rollback(r0, (int64_t)rs, groups, log + 3 * pod0, n_log, out_pod + pod0,
                   groups[g1 - 1].pod0 + groups[g1 - 1].count - pod0);
    __syncthreads();   // the owners read their places again
  }
  return ok;
}

// One workgroup per active domain a = blockIdx.x; a workgroup whose segment is the other instance's leaves at once.
// bk: the book and the call's rows (cnt and sub parallel to the segments' places; b, sb unset).  decisions: every
// workgroup adds the takes it made, once.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void skew_domains_kernel(
    const PlaceGroup* __restrict__ groups, const PlaceJob* __restrict__ jobs, const int32_t* __restrict__ job_start,
    PlaceSegs sg, SkewRows bk, int64_t* __restrict__ res, int64_t stride, uint32_t id_base, int dry_run,
    int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status, int32_t* __restrict__ log,
    unsigned long long* __restrict__ decisions) {
  __shared__ SkewMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= SK_LDS_NODES) != IN_LDS) return;
  int64_t* const seg = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs, const SkewRows& rw) {
    int par = 0;
    uint32_t dec = 0;
    for (int ji = job_start[a]; ji < job_start[a + 1]; ++ji) {
      const PlaceJob pj = jobs[ji];
      const bool ok = pj.g0 == pj.g1 ||   // no groups: placed
                      skew_job(r0, ids, rs, rw, n, mn, par, dec, groups, pj.g0, pj.g1, out_pod, log);
      if (tid == 0) out_status[pj.job] = ok ? 0 : 1;
    }
    if (tid == 0) atomicAdd(decisions, (unsigned long long)dec);
    if (dry_run) return;
    for (int i = tid; i < n; i += PL_THREADS) {
      const int64_t l = (int64_t)(ids[i] - id_base);   // < Ns: the fill kernel wrote id_base + local
#pragma unroll
      for (int d = 0; d < D; ++d) res[d * stride + l] = r0[d * rs + i];
    }
  };
  SkewRows rw = bk;
  rw.b = (uint32_t)b;
  if constexpr (IN_LDS) {
    __shared__ SkewShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
#pragma unroll
      for (int d = 0; d < D; ++d) sh.r[d][i] = seg[d * ss + i];
      sh.lab[i] = gid[ss + i];
      sh.gid[i] = gid[i];
      sh.sub[i] = bk.sub ? bk.sub[b + i] - (uint32_t)b : (uint32_t)i;   // no row: no group of the call is constrained
    }
    rw.cnt = sh.cnt;
    rw.sub = sh.sub;
    rw.sb = 0;
    run(sh.r[0], sh.gid, std::integral_constant<int, SkewShared::N>(), rw);
  } else {
    rw.cnt = bk.cnt + b;
    rw.sub = bk.sub ? bk.sub + b : nullptr;
    rw.sb = (uint32_t)b;
    run(seg, gid, ss, rw);
  }
}

}  // namespace

hipError_t launch_skew_domains(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* job_start,
                               int A, const PlaceSegs& segs, const int32_t* island, int64_t Ns, const int32_t* leaf_sd,
                               const int32_t* skew, const int32_t* book_off, const int32_t* book, bool constrained,
                               uint32_t* sub_row, uint32_t* cnt_row, int32_t* where, int64_t n_keys, int64_t* res,
                               int64_t stride, uint64_t id_base, bool dry_run, int32_t* out_pod, int32_t* out_status,
                               int32_t* log, unsigned long long* decisions) {
  if (A <= 0) return hipSuccess;
  if (A > DM_MAX_DOMAINS || Ns < 0 || Ns > (int64_t(1) << 24) || n_keys < 0 || n_keys > INT32_MAX || !skew || !book_off ||
      !decisions || !sub_row || !cnt_row)
    return hipErrorInvalidValue;
  if (constrained) {
    if (!where || !island) return hipErrorInvalidValue;
    const unsigned kb = (unsigned)((n_keys + SKP_THREADS - 1) / SKP_THREADS);
    const unsigned pb = (unsigned)((Ns + SKP_THREADS - 1) / SKP_THREADS);
    if (kb > 0) hipLaunchKernelGGL(skew_clear_kernel, dim3(kb), dim3(SKP_THREADS), 0, s, where, n_keys);
    if (pb > 0) {
      hipLaunchKernelGGL(skew_first_kernel, dim3(pb), dim3(SKP_THREADS), 0, s, segs, A, island, (uint32_t)id_base, leaf_sd,
                         n_keys, where);
      hipLaunchKernelGGL(skew_sub_kernel, dim3(pb), dim3(SKP_THREADS), 0, s, segs, A, island, (uint32_t)id_base, leaf_sd,
                         n_keys, where, sub_row);
    }
  }
  SkewRows bk;
  bk.cnt = cnt_row;
  bk.sub = constrained ? sub_row : nullptr;
  bk.b = bk.sb = 0;
  bk.skew = skew;
  bk.book_off = book_off;
  bk.book = book;
  bk.where = where;
  bk.n_keys = (uint32_t)n_keys;
  bk.id_base = leaf_sd ? 0u : (uint32_t)id_base;   // a node's key is its local id, a domain's its own
  hipLaunchKernelGGL(skew_domains_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     bk, res, stride, (uint32_t)id_base, dry_run ? 1 : 0, out_pod, out_status, log, decisions);
  hipLaunchKernelGGL(skew_domains_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     bk, res, stride, (uint32_t)id_base, dry_run ? 1 : 0, out_pod, out_status, log, decisions);
  return hipGetLastError();
}

}  // namespace pe
