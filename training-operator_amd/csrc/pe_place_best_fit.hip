// Best-fit placement of a batch over candidate domains (pe_place_best_fit_domains): every job, in (priority desc,
// index asc) order, goes to the candidate domain that fits it and has the fewest slots for its reference group,
// against the residuals as the earlier jobs left them.  First fit's frame (pe_place.hip: member lists, compact
// segments that stay the domains' working residuals from round to round, one workgroup per active domain, rounds
// of one launch each, nobody waits for anybody), with a job's choice split in two steps that no workgroup needs
// another one for:
//
// EVALUATE.  The head (j, p) of domain a's queue has the lowest rank among the entries still open there, so every
// earlier job that names a is settled and a's segment is what the sequential rule shows job j.  The workgroup sums
// cap(n) of j's reference group over the segment -- one block reduction, take_of's division per fitting node -- and
// runs j's groups through pe_place_step.h's walk on a COPY of the segment: the LDS instance walks its staged state
// and throws it away (what it placed for real earlier in the round went back to the segment first), the in-place
// instance copies the four rows to the call's shadow array.  Nothing is logged and nothing rolled back: a job's log
// range is one per job, and several domains evaluate one job in the same round.  ev_slots[p] = slots or -1, then
// ev_round[p] = the round; the entry stays the head and the round is over for this domain.
//
// DECIDE.  A head evaluated in an earlier round.  The first wave reads the stamps and the slots of the job's kept
// pairs; a stamp of 0 or of this very round counts as missing -- so what a workgroup sees does not depend on which
// workgroup ran first -- and a missing one ends the round for this domain.  Otherwise every domain of the job
// computes the same argmin of (slots, p) over the fitting pairs, from words written in earlier launches.  The
// domain of that pair places the job for real (place_job: the segment is as it was at the evaluation, so it is
// placed), the others pass the entry by, and where no pair fits the domain of the job's smallest kept pair takes
// the job off the unsettled count.  Either way the workgroup goes on to its next head in the same round.
//
// Each round evaluates a pair or settles a job, so n_pairs + n_jobs rounds settle every batch.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_place_job.h"
#include "pe_place_step.h"

namespace pe {

namespace {

struct BestHead {            // what the workgroup knows of its head: two sets used in turn, one barrier per entry
  uint64_t sum[PL_WAVES];    // the waves' shares of slots(p): at most one evaluation per launch
  uint64_t slots[2];         // the job's tightest fitting pair and its slots; NO_KEY and ~0: no pair fits
  uint32_t pair[2];
  uint32_t mine[2];          // the stamp of the head's own pair
  uint32_t missing[2];       // some kept pair of the job has no stamp from an earlier round
};
// four workgroups per CU: 160 KiB of LDS, 40 KiB each
static_assert(sizeof(PlaceShared) + sizeof(PlaceMin) + sizeof(BestHead) <= 40 * 1024, "PL_LDS_NODES: lower the limit");

template <class T>
__device__ __forceinline__ T peek(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slots of group gr on the n places of w0[d * ws + i] with labels lab: the sum of cap(n) as pe_gang_capacity
// defines it, PE_NEED_ISLAND masked off.  The same on every thread; one barrier.
template <class Stride>
__device__ __forceinline__ uint64_t best_slots(const int64_t* w0, Stride ws, const uint32_t* lab, int n,
                                               const PlaceGroup& gr, BestHead& hd) {
  const int tid = threadIdx.x;
  const uint32_t need = gr.need & ~NEED_ISLAND;
  const int64_t q0 = gr.q[0], q1 = gr.q[1], q2 = gr.q[2], q3 = gr.q[3];
  uint64_t sum = 0;
  for (int i = tid; i < n; i += PL_THREADS) {
    const int64_t x0 = w0[i], x1 = w0[ws + i], x2 = w0[2 * ws + i], x3 = w0[3 * ws + i];
    if ((lab[i] & need) == need && q0 <= x0 && q1 <= x1 && q2 <= x2 && q3 <= x3)
      sum += take_of(x0, x1, x2, x3, q0, q1, q2, q3, (uint32_t)CP_CAP_MAX);
  }
  sum = group_sum_u64(sum, 64);
  if ((tid & 63) == 0) hd.sum[tid >> 6] = sum;
  __syncthreads();
  sum = 0;
#pragma unroll
  for (int w = 0; w < PL_WAVES; ++w) sum += hd.sum[w];
  return sum;
}

// Would groups [g0, g1) be placed on the n places of w0?  w0 is a copy: what the walk takes stays taken.
template <class Stride>
__device__ __forceinline__ bool best_what_if(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab, int n,
                                             PlaceMin& mn, int& par, const PlaceGroup* __restrict__ groups, int g0,
                                             int g1) {
  uint32_t left;
  return place_groups(w0, ws, gid, lab, n, mn, par, groups, g0, g1, left,
                      [](int, const PlaceGroup&, const PlaceChoice&, uint32_t) {}) == g1;
}

// One round of active domain a on its n nodes.  IN_LDS: r0 / gid are the workgroup's LDS rows (stride rs), loaded
// from the segment seg / sgid (stride ss) before the first use and written back after a placement; else r0 == seg,
// gid == sgid, rs == ss and `shadow` (stride ss) takes the copy an evaluation walks.
template <bool IN_LDS, class Stride>
__device__ __forceinline__ void best_fit_queue(int64_t* r0, uint32_t* gid, Stride rs, int64_t* seg, const uint32_t* sgid,
                                               int64_t ss, int64_t* shadow, int n, PlaceMin& mn, BestHead& hd,
                                               const PlaceGroup* __restrict__ groups,
                                               const BestFitJob* __restrict__ jobs, const int32_t* __restrict__ kept,
                                               const BestFitEntry* __restrict__ queue, int cur, int end, int a,
                                               uint32_t round, const BestFitState& st, int32_t* __restrict__ out_pod,
                                               int32_t* __restrict__ out_status, int32_t* __restrict__ out_pair,
                                               int32_t* __restrict__ log) {
  const int tid = threadIdx.x, lane = tid & 63;
  int par = 0, hp = 0;
  bool staged = !IN_LDS, dirty = false;
  const auto stage = [&]() {   // thread i mod PL_THREADS owns place i: no barrier
    if (staged) return;
    staged = true;
    for (int i = tid; i < n; i += PL_THREADS) {
#pragma unroll
      for (int d = 0; d < D; ++d) r0[d * rs + i] = seg[d * ss + i];
      gid[rs + i] = sgid[ss + i];
      gid[i] = sgid[i];
    }
  };
  const auto flush = [&]() {
    if (!IN_LDS || !dirty) return;
    dirty = false;
    for (int i = tid; i < n; i += PL_THREADS) {
#pragma unroll
      for (int d = 0; d < D; ++d) seg[d * ss + i] = r0[d * rs + i];
    }
  };
  for (; cur < end; ++cur) {
    const BestFitEntry e = queue[cur];
    const BestFitJob bj = jobs[e.job];
    if (tid < 64) {   // the job's kept pairs, ascending per lane: a strict < keeps the smaller p
      uint64_t bs = NO_KEY;
      uint32_t bp = ~0u;
      bool miss = false;
      for (int k = bj.k0 + lane; k < bj.k1; k += 64) {
        const int32_t p = kept[k];
        const uint32_t stamp = peek(&st.ev_round[p]);
        if (stamp == 0 || stamp == round) {
          miss = true;
          continue;
        }
        const long long s = peek(&st.ev_slots[p]);
        if (s >= 0 && (uint64_t)s < bs) {
          bs = (uint64_t)s;
          bp = (uint32_t)p;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint64_t os = __shfl_xor(bs, o, 64);
        const uint32_t op = __shfl_xor(bp, o, 64);
        if (os < bs || (os == bs && op < bp)) {
          bs = os;
          bp = op;
        }
      }
      const bool any = __any(miss);
      if (lane == 0) {
        hd.slots[hp] = bs;
        hd.pair[hp] = bp;
        hd.missing[hp] = any;
        hd.mine[hp] = peek(&st.ev_round[e.pair]);
      }
    }
    __syncthreads();
    const uint32_t mine = hd.mine[hp], win = hd.pair[hp];
    const bool missing = hd.missing[hp] != 0;
    hp ^= 1;
    if (mine == 0) {   // EVALUATE, on a copy; the round ends here
      int64_t* w0 = r0;
      if constexpr (IN_LDS) {
        flush();
        stage();
      } else {
        w0 = shadow;
        for (int i = tid; i < n; i += PL_THREADS) {
#pragma unroll
          for (int d = 0; d < D; ++d) w0[d * ss + i] = seg[d * ss + i];
        }
      }
      const uint64_t slots = bj.ref >= 0 ? best_slots(w0, rs, gid + rs, n, groups[bj.ref], hd) : 0;
      const bool fits = bj.g0 == bj.g1 || best_what_if(w0, rs, gid, gid + rs, n, mn, par, groups, bj.g0, bj.g1);
      if (tid == 0) {
        st.ev_slots[e.pair] = fits ? (long long)slots : -1;
        __hip_atomic_store(&st.ev_round[e.pair], round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      break;
    }
    if (missing) break;   // DECIDE, once every kept pair has its stamp
    if (win == (uint32_t)e.pair) {
      stage();
      const bool ok = bj.g0 == bj.g1 || place_job(r0, gid, rs, n, mn, par, groups, bj.g0, bj.g1, out_pod, log);
      dirty = true;
      if (tid == 0) {
        if (ok) {   // as evaluated: the segment has not changed since
          out_status[e.job] = 0;
          out_pair[e.job] = e.pair;
        }
        atomicSub(st.open, 1u);
      }
    } else if (win == ~0u && kept[bj.k0] == e.pair) {   // fits nowhere: settled by one of its domains
      if (tid == 0) atomicSub(st.open, 1u);
    }
  }
  flush();
  if (tid == 0) st.cursor[a] = cur;
}

// IN_LDS as for first_fit_round_kernel: the segments of at most PL_LDS_NODES nodes in LDS, the larger ones in place.
template <bool IN_LDS>
__global__ __launch_bounds__(PL_THREADS) void best_fit_round_kernel(
    const PlaceGroup* __restrict__ groups, const BestFitJob* __restrict__ jobs, const int32_t* __restrict__ kept,
    const int32_t* __restrict__ q_start, const BestFitEntry* __restrict__ queue, PlaceSegs sg, int64_t* shadow,
    uint32_t round, BestFitState st, int32_t* __restrict__ out_pod, int32_t* __restrict__ out_status,
    int32_t* __restrict__ out_pair, int32_t* __restrict__ log) {
  __shared__ PlaceMin mn;
  __shared__ BestHead hd;
  const int a = blockIdx.x;
  const int cur = st.cursor[a], end = q_start[a + 1];   // the cursor is this workgroup's own, round after round
  if (cur >= end) return;
  const int b = sg.seg_off[a], n = sg.seg_off[a + 1] - b;
  if ((n <= PL_LDS_NODES) != IN_LDS) return;
  int64_t* const seg = sg.res + b;
  const int64_t ss = sg.seg_stride;
  uint32_t* const sgid = sg.gid + b;
  if constexpr (IN_LDS) {
    __shared__ PlaceShared sh;
    best_fit_queue<true>(sh.r[0], sh.gid, std::integral_constant<int, PL_LDS_NODES>(), seg, sgid, ss, nullptr, n, mn, hd,
                         groups, jobs, kept, queue, cur, end, a, round, st, out_pod, out_status, out_pair, log);
  } else {
    best_fit_queue<false>(seg, sgid, ss, seg, sgid, ss, shadow + b, n, mn, hd, groups, jobs, kept, queue, cur, end, a,
                          round, st, out_pod, out_status, out_pair, log);
  }
}

}  // namespace

hipError_t launch_best_fit_round(hipStream_t s, const PlaceGroup* groups, const BestFitJob* jobs, const int32_t* kept,
                                 const int32_t* q_start, const BestFitEntry* queue, int A, const PlaceSegs& segs,
                                 int64_t* shadow, int kinds, uint32_t round, const BestFitState& st, int32_t* out_pod,
                                 int32_t* out_status, int32_t* out_pair, int32_t* log) {
  if (A <= 0) return hipSuccess;
  if (round == 0 || A > DM_MAX_DOMAINS || ((kinds & FF_LARGE) && !shadow)) return hipErrorInvalidValue;   // 0: no stamp
  if (kinds & FF_SMALL)
    hipLaunchKernelGGL(best_fit_round_kernel<true>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, kept, q_start,
                       queue, segs, shadow, round, st, out_pod, out_status, out_pair, log);
  if (kinds & FF_LARGE)
    hipLaunchKernelGGL(best_fit_round_kernel<false>, dim3((unsigned)A), dim3(PL_THREADS), 0, s, groups, jobs, kept, q_start,
                       queue, segs, shadow, round, st, out_pod, out_status, out_pair, log);
  return hipGetLastError();
}

}  // namespace pe
