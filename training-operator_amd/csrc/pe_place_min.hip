// MinMember first, the rest as fits (pe_place_min_member_domains): pe_place_greedy_domains' scheme -- one
// workgroup per ACTIVE domain, all domains in parallel, the member lists from launch_place_members (pe_place.hip)
// -- with every job in two phases.
//
// Phase 1 is place_job (pe_place_job.h) as it stands, on the job's MANDATORY records: all-or-nothing, its log of
// (place, group, pods) entries and its rollback unchanged.  The mandatory pods of a job are the first pods of its
// slot range, so the plan (pe_place_min_plan.h) numbers them a second time without the optional ones: the log
// lives in that numbering (3 int32 per mandatory pod, whatever the optional counts are) and the pod stores go
// through a shifted out_pod to the slots among all slots.  A job that fails phase 1 gets -1 in ALL its slots and
// leaves its groups' counts at the 0 the caller filled them with; phase 2 is not tried.
//
// Phase 2 (place_optional, this file's) walks the job's OPTIONAL records in order, each through the one-group
// walk of pe_place_step.h (place_group): t = min(pods left, floor(res / q)) pods per decision, so a count of
// 2^31 - 1 with a zero request is one decision; an optional island group is one decision for count x request or
// nothing.  The first
// decision of a group that finds no node ends that group: its remaining slots become -1 and the walk goes on with
// the next group.  Nothing of phase 2 is logged or rolled back.  Between decisions the working state is read and
// written by its owner thread only (thread i mod PL_THREADS owns place i), as in phase 1, so phase 2 adds no
// barrier of its own; after a rollback place_job has already synchronised.
//
// The working state lives in LDS for segments up to PL_LDS_NODES nodes and in the global segment beyond: two
// instances, as place_domains_kernel, on the same frame (place_frame, pe_place_job.h).
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_place_step.h"

namespace pe {

namespace {

// The optional pods of one placed job: group g's request, need and mandatory count from groups[g], its optional share
// from opt[g].  Writes the optional slots (node or -1) and out_group_pods[g] for every group of the job.
template <class Stride>
__device__ __forceinline__ void place_optional(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn, int& par,
                                               const PlaceGroup* __restrict__ groups, const PlaceMinOpt* __restrict__ opt,
                                               int g0, int g1, int32_t* __restrict__ out_pod,
                                               int32_t* __restrict__ out_group_pods) {
  const int tid = threadIdx.x;
  for (int g = g0; g < g1; ++g) {
    const PlaceMinOpt op = opt[g];
    PlaceGroup gr = groups[g];
    const int32_t mand = gr.count;
    gr.count = op.count;   // an optional island group is optional as a whole: its unit is op.count x request
    // a group that finds no node ends there, and the walk goes on with the next: its pods left stay pending
    const uint32_t left = place_group(r0, rs, gid, gid + rs, n, mn, par, gr, [&](const PlaceChoice& c, uint32_t done) {
      const int32_t node = (int32_t)(c.klo & 0xFFFFFFu);
      const int64_t slot = op.pod0 + done;   // slot + t <= the group's end
      for (int64_t p = slot + tid; p < slot + c.t; p += PL_THREADS) out_pod[p] = node;
    });
    const int32_t placed = op.count > 0 ? op.count - (int32_t)left : 0;
    for (int64_t p = op.pod0 + placed + tid; p < op.pod0 + placed + left; p += PL_THREADS) out_pod[p] = -1;
    // mandatory + optional placed <= the group's count <= 2^31 - 1
    if (tid == 0) out_group_pods[g] = mand + placed;
  }
}

// One domain's jobs jobs[j0 .. j1), in that order, on its n nodes (the working state as for place_job).
template <class Stride>
__device__ __forceinline__ void place_min_domain(int64_t* r0, const uint32_t* gid, Stride rs, int n, PlaceMin& mn,
                                                 const PlaceGroup* __restrict__ groups,
                                                 const PlaceMinOpt* __restrict__ opt, const PlaceMinJob* __restrict__ jobs,
                                                 int j0, int j1, int32_t* __restrict__ out_pod,
                                                 int32_t* __restrict__ out_status, int32_t* __restrict__ out_group_pods,
                                                 int32_t* __restrict__ log) {
  const int tid = threadIdx.x;
  int par = 0;
  for (int ji = j0; ji < j1; ++ji) {
    const PlaceMinJob pj = jobs[ji];
    // phase 1: the mandatory records, whose slots are numbered without the optional ones; a job without a
    // mandatory pod is placed
    const bool ok =
        pj.gm == pj.g0 || place_job(r0, gid, rs, n, mn, par, groups, pj.g0, pj.gm, out_pod + pj.shift, log);
    if (tid == 0) out_status[pj.job] = ok ? 0 : 1;
    if (!ok) {   // gm > g0: the job has groups.  Every slot -1 (the rollback wrote the mandatory ones); the counts stay 0
      int32_t* const mine = out_pod + (groups[pj.g0].pod0 + pj.shift);
      for (int64_t p = tid; p < pj.pods; p += PL_THREADS) mine[p] = -1;
      continue;
    }
    place_optional(r0, gid, rs, n, mn, par, groups, opt, pj.g0, pj.g1, out_pod, out_group_pods);
  }
}

// place_frame around place_min_domain, IN_LDS as for place_domains_kernel.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void place_min_domains_kernel(
    const PlaceGroup* __restrict__ groups, const PlaceMinOpt* __restrict__ opt, const PlaceMinJob* __restrict__ jobs,
    const int32_t* __restrict__ job_start, PlaceSegs sg, int64_t* __restrict__ res, int64_t stride, uint32_t id_base,
    int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status, int32_t* __restrict__ out_group_pods,
    int32_t* __restrict__ log) {
  place_frame<IN_LDS>(sg, res, stride, id_base, [&](int64_t* r0, const uint32_t* gid, auto rs, int n, PlaceMin& mn) {
    const int a = blockIdx.x;
    place_min_domain(r0, gid, rs, n, mn, groups, opt, jobs, job_start[a], job_start[a + 1], out_pod, out_status,
                     out_group_pods, log);
  });
}

}  // namespace

hipError_t launch_place_min_domains(hipStream_t s, const PlaceGroup* groups, const PlaceMinOpt* opt,
                                    const PlaceMinJob* jobs, const int32_t* job_start, int A, const PlaceSegs& segs,
                                    int64_t* res, int64_t stride, uint64_t id_base, int32_t* out_pod, int32_t* out_status,
                                    int32_t* out_group_pods, int32_t* log) {
  if (A <= 0) return hipSuccess;
  hipLaunchKernelGGL(place_min_domains_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, opt, jobs,
                     job_start, segs, res, stride, (uint32_t)id_base, out_pod, out_status, out_group_pods, log);
  hipLaunchKernelGGL(place_min_domains_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, opt, jobs,
                     job_start, segs, res, stride, (uint32_t)id_base, out_pod, out_status, out_group_pods, log);
  return hipGetLastError();
}

}  // namespace pe
