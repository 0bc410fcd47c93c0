// Least-allocated gang placement inside a chosen topology domain (pe_place_least_domains): pe_place.hip's scheme --
// one workgroup per active domain, its jobs in plan order on the domain's compact segment -- with pe_least_step.h's
// decision, which spreads: each pod goes to the fitting node that keeps the most room.  Why the packing calls'
// take-many does not carry over, and the two kinds of decision that replace it (a ROUND of one pod on each of
// several nodes, a RUN of several pods on one node), are stated in pe_least_step.h.
//
// least_domains_kernel<IN_LDS>: two instances.  The working state of a place is pe_place.hip's 40 B (four residuals,
// labels, id); a round's list of keys costs 8 B per place more, so the instance that stages the segment in LDS has
// a limit of its own, the largest segment that keeps the workgroup within the 40 KiB at which four of them share a
// CU (pe_kernels.h: LS_LDS_NODES).  A larger segment is worked on in place on the compact global segment, with the
// list in the call's scratch.  The job frame is place_job's: a log of (place, group, pods) entries in the job's own
// pod range -- a run writes one entry, a round one per pod, so entries <= pods placed still holds --, place_rollback
// for a failed job.  Within a group the pod slots are in the order of the pod-by-pod rule: a run fills the next t
// slots with its node, a round's members write the slot of their rank.  A dry run skips the write-back to the live
// residuals and nothing else.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_least_step.h"
#include "pe_place_job.h"

namespace pe {

namespace {

struct LeastShared {
  static constexpr int N = LS_LDS_NODES;
  int64_t r[D][N];
  uint64_t list[N];
  uint32_t gid[N], lab[N];
};
static_assert(sizeof(LeastShared) + sizeof(LeastMin) <= 40 * 1024 &&
                  sizeof(LeastShared) + sizeof(LeastMin) + 48 > 40 * 1024,
              "LS_LDS_NODES: the largest segment within 40 KiB");

// One job (groups [g0, g1), g0 < g1) on a domain's n nodes, all or nothing: whether it is placed, the same on every
// thread.  The working state is r0[d * rs + i] (written), gid[i] and labels gid[rs + i]; list: n keys of scratch.
// par, dec: the decisions' parity and their count, carried from job to job.
template <bool IN_LDS, class Stride>
__device__ __forceinline__ bool least_job(int64_t* r0, const uint32_t* gid, Stride rs, int n, LeastMin& mn, int& par,
                                          uint32_t& dec, uint64_t* list, const PlaceGroup* __restrict__ groups, int g0,
                                          int g1, int32_t* __restrict__ out_pod, int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  int64_t* const r1 = r0 + rs;
  int64_t* const r2 = r1 + rs;
  int64_t* const r3 = r2 + rs;
  const uint32_t* const lab = gid + rs;
  const int64_t pod0 = groups[g0].pod0;   // the job's pod slots: [pod0, the last group's pod0 + count)
  int64_t n_log = 0;                      // entries of this job, at log[3 pod0 ..]; <= the pods it placed
  bool ok = true;
  for (int g = g0; g < g1 && ok; ++g) {
    const PlaceGroup gr = groups[g];
    if (gr.count <= 0) continue;
    const bool unit = (gr.need & NEED_ISLAND) != 0;
    int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
    uint32_t left = (uint32_t)gr.count;
    if (unit && !island_request(gr, s0, s1, s2, s3)) {   // an overflowing product fits nowhere
      ok = false;
      break;
    }
    while (left > 0) {
      const LeastChoice c = least_decide(r0, r1, r2, r3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, mn, par);
      const int set = par;
      par ^= 1;
      ++dec;
      if (c.none()) {   // no node of the domain fits
        ok = false;
        break;
      }
      const int64_t slot = gr.pod0 + ((uint32_t)gr.count - left);   // slot + the pods of this decision <= pod1 <= P
      int32_t* const entry = log + 3 * (pod0 + n_log);
      uint32_t t = 0;
      if (!unit && c.round()) {
        t = least_round<!IN_LDS>(r0, r1, r2, r3, gid, lab, n, s0, s1, s2, s3, gr.need, c, left, list, mn, set,
                                 [&](int i, uint32_t rank, uint32_t node) {
                                   out_pod[slot + rank] = (int32_t)node;
                                   int32_t* const e = entry + 3 * rank;
                                   e[0] = i;
                                   e[1] = g;
                                   e[2] = 1;
                                 });
        n_log += t;
      }
      if (t == 0) {   // a run; an island group: one unit of s = count x request, logged with its pods
        t = unit ? left : least_run_len(c, s0, s1, s2, s3, gr.need, left);
        const int64_t m = unit ? 1 : (int64_t)t;
        if ((c.at & (PL_THREADS - 1)) == (uint32_t)tid) {
          r0[c.at] = c.r0 - m * s0;
          r1[c.at] = c.r1 - m * s1;
          r2[c.at] = c.r2 - m * s2;
          r3[c.at] = c.r3 - m * s3;
        }
        if (tid == 0) {
          entry[0] = (int32_t)c.at;
          entry[1] = g;
          entry[2] = (int32_t)t;
        }
        ++n_log;
        const int32_t node = (int32_t)(c.k1 & 0xFFFFFFu);
        for (int64_t p = slot + tid; p < slot + t; p += PL_THREADS) out_pod[p] = node;
      }
      left -= t;
    }
  }
  if (!ok) {
    __syncthreads();   // every update, pod store and log entry of this job lies before this barrier
    place_rollback(r0, (int64_t)rs, groups, log + 3 * pod0, n_log, out_pod + pod0,
                   groups[g1 - 1].pod0 + groups[g1 - 1].count - pod0);
    __syncthreads();   // the owners read their places again
  }
  return ok;
}

// One workgroup per active domain a = blockIdx.x; a workgroup whose segment is the other instance's leaves at once.
// lists: the in-place instance's keys, parallel to the segments' places.  decisions: every workgroup adds the
// decisions it made, once.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void least_domains_kernel(
    const PlaceGroup* __restrict__ groups, const PlaceJob* __restrict__ jobs, const int32_t* __restrict__ job_start,
    PlaceSegs sg, uint64_t* __restrict__ lists, int64_t* __restrict__ res, int64_t stride, uint32_t id_base, int dry_run,
    int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status, int32_t* __restrict__ log,
    unsigned long long* __restrict__ decisions) {
  __shared__ LeastMin mn;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= LS_LDS_NODES) != IN_LDS) return;
  int64_t* const seg = sg.res + b;
  const int64_t ss = sg.seg_stride;
  const uint32_t* const gid = sg.gid + b;
  if (tid == 0) mn.cnt[0] = mn.cnt[1] = 0;   // before the first decision's barrier, used after it
  const auto run = [&](int64_t* r0, const uint32_t* ids, auto rs, uint64_t* list) {
    int par = 0;
    uint32_t dec = 0;
    for (int ji = job_start[a]; ji < job_start[a + 1]; ++ji) {
      const PlaceJob pj = jobs[ji];
      const bool ok = pj.g0 == pj.g1 ||   // no groups: placed
                      least_job<IN_LDS>(r0, ids, rs, n, mn, par, dec, list, groups, pj.g0, pj.g1, out_pod, log);
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
  if constexpr (IN_LDS) {
    __shared__ LeastShared sh;
    for (int i = tid; i < n; i += PL_THREADS) {   // thread i mod PL_THREADS owns place i: no barrier
#pragma unroll
      for (int d = 0; d < D; ++d) sh.r[d][i] = seg[d * ss + i];
      sh.lab[i] = gid[ss + i];
      sh.gid[i] = gid[i];
    }
    run(sh.r[0], sh.gid, std::integral_constant<int, LeastShared::N>(), sh.list);
  } else {
    run(seg, gid, ss, lists + b);
  }
}

}  // namespace

hipError_t launch_least_domains(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* job_start,
                                int A, const PlaceSegs& segs, uint64_t* lists, int64_t* res, int64_t stride,
                                uint64_t id_base, bool dry_run, int32_t* out_pod, int32_t* out_status, int32_t* log,
                                unsigned long long* decisions) {
  if (A <= 0) return hipSuccess;
  if (A > DM_MAX_DOMAINS || !lists || !decisions) return hipErrorInvalidValue;
  hipLaunchKernelGGL(least_domains_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     lists, res, stride, (uint32_t)id_base, dry_run ? 1 : 0, out_pod, out_status, log, decisions);
  hipLaunchKernelGGL(least_domains_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, job_start, segs,
                     lists, res, stride, (uint32_t)id_base, dry_run ? 1 : 0, out_pod, out_status, log, decisions);
  return hipGetLastError();
}

}  // namespace pe
