// The least-allocated rule inside a domain's segment (pe_place_least_domains; device code only): one DECISION in
// its two kinds, beside pe_place_step.h, whose key arithmetic, take_of and island_request it reuses and whose own
// decision stays as it is.
//
// The rule pod by pod: a pod goes to the fitting node with the LARGEST Appendix-B score after the pod, ties to the
// lowest id; as an argmin, to the node with the smallest
//   least_key(n) = fit ? ((SCORE_MAX - score) << 24) | gid : NO_KEY          (fit, score: node_key's)
// A pod that lands on node n lowers n's leftover, so n's score falls or stays saturated and n's least_key RISES or
// stays: pe_place_step.h's take-many argument fails, the chosen node loses the argmin as it fills.  What holds
// instead, with key(n) the key now and after(n) the key once n has taken one pod (NO_KEY if it then no longer fits):
//
//   k1, k2   the smallest and the second smallest key(n)
//   theta    the smallest after(n)
//
// ROUND (k2 < theta): W = { n : key(n) < theta } has two members or more, and the min(|W|, left) members of W with
// the smallest keys take ONE pod each, in ascending key order.  Exact: after any prefix of W (by key) has taken its
// pod those nodes sit at after(n) >= theta, every node outside W was at theta or above already, and the next member
// of W is still below theta -- so it is the argmin of the pod-by-pod rule.  On a levelled rack one decision places a
// whole layer.
// RUN (otherwise): only the argmin node is below theta, or it is not below it either (key == after: a saturated
// score or a zero request).  No other node's key moves, so the argmin node takes pods for as long as its key stays
// below k2 and it fits: t = the largest t <= min(left, take_of) with least_key after i pods < k2 for every i < t.
// The key after i pods does not fall as i grows, so t is found by search on exact integer evaluations of the key;
// the 64 lanes of a wave probe 64 values of i at once (two steps for any t below 4096, six for 2^31).
//
// One block reduction per decision -- a wave butterfly over (k1, k2, theta, the argmin's place), then one
// cross-wave step through LDS, as place_decide -- and the argmin's four residuals ride along in the waves' slots, so
// that a run needs no second barrier: every wave finds the same t.  A round needs the members' ranks by key: the
// members append their keys to a list through an LDS counter, the block passes a second barrier, and every member
// counts the keys below its own.  The rank is its pod slot and its log entry; the owner takes the request off its
// own place, so thread i mod PL_THREADS stays the only one that touches place i.
#pragma once
#include "pe_place_step.h"

namespace pe {

// fit and score are node_key's; SCORE_MAX - score is score with its 40 bits turned round.
__device__ __forceinline__ uint64_t least_key(int64_t r0, int64_t r1, int64_t r2, int64_t r3, uint32_t lab, int64_t q0,
                                              int64_t q1, int64_t q2, int64_t q3, uint32_t need, uint64_t gid) {
  const bool fit = ((lab & need) == need) & (q0 <= r0) & (q1 <= r1) & (q2 <= r2) & (q3 <= r3);
  const uint64_t k = node_key(r0, r1, r2, r3, lab, q0, q1, q2, q3, need, gid);
  return fit ? (k ^ (SCORE_MAX << 24)) : NO_KEY;
}

struct LeastMin {   // the waves' results of a decision, two sets used in turn, and the rounds' list counters
  uint64_t k1[2][PL_WAVES], k2[2][PL_WAVES], th[2][PL_WAVES];
  int64_t r[2][PL_WAVES][D];   // the residuals of the wave's argmin place
  uint32_t at[2][PL_WAVES];
  uint32_t cnt[2];
};

// The block's view of a decision, the same on every thread: k1 (NO_KEY: no node of the segment fits), k2, theta,
// the argmin's place and its residuals.
struct LeastChoice {
  uint64_t k1, k2, th;
  int64_t r0, r1, r2, r3;
  uint32_t at;
  __device__ __forceinline__ bool none() const { return k1 == NO_KEY; }
  __device__ __forceinline__ bool round() const { return k2 < th; }
};

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);   // the builtin's int would sign-extend
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// The decision's reduction for request s among the n places of the working state.  unit: an island group, which
// needs the argmin alone (theta is left at NO_KEY).  `par` names the set of `mn` to use; the caller alternates it.
// cnt[par] is zero on return and stays so until the round of this decision appends.  Called by the whole workgroup.
__device__ __forceinline__ LeastChoice least_decide(const int64_t* r0, const int64_t* r1, const int64_t* r2,
                                                    const int64_t* r3, const uint32_t* gid, const uint32_t* lab, int n,
                                                    int64_t s0, int64_t s1, int64_t s2, int64_t s3, uint32_t need,
                                                    bool unit, LeastMin& mn, int par) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t a1 = NO_KEY, a2 = NO_KEY, th = NO_KEY;
  uint32_t ai = 0;
  for (int i = tid; i < n; i += PL_THREADS) {
    const int64_t x0 = r0[i], x1 = r1[i], x2 = r2[i], x3 = r3[i];
    const uint32_t l = lab[i], g = gid[i];
    const uint64_t k = least_key(x0, x1, x2, x3, l, s0, s1, s2, s3, need, g);
    if (!unit && k != NO_KEY)   // x - s >= 0 in every dimension: the node fits
      th = min(th, least_key(x0 - s0, x1 - s1, x2 - s2, x3 - s3, l, s0, s1, s2, s3, need, g));
    if (k < a1) {
      a2 = a1;
      a1 = k;
      ai = (uint32_t)i;
    } else {
      a2 = min(a2, k);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // the lanes' sets are disjoint at every step
    const uint64_t o1 = __shfl_xor(a1, o, 64), o2 = __shfl_xor(a2, o, 64);
    const uint32_t oi = __shfl_xor(ai, o, 64);
    th = min(th, (uint64_t)__shfl_xor(th, o, 64));
    const uint64_t m2 = min(a2, o2);
    if (o1 < a1) {
      a2 = min(a1, m2);
      a1 = o1;
      ai = oi;
    } else {
      a2 = min(o1, m2);
    }
  }
  if (lane == 0) {
    mn.k1[par][wave] = a1;
    mn.k2[par][wave] = a2;
    mn.th[par][wave] = th;
    mn.at[par][wave] = ai;
  }
  if (a1 != NO_KEY && (ai & 63u) == (uint32_t)lane) {   // the wave's argmin is a place of this lane: its owner reads it
    mn.r[par][wave][0] = r0[ai];
    mn.r[par][wave][1] = r1[ai];
    mn.r[par][wave][2] = r2[ai];
    mn.r[par][wave][3] = r3[ai];
  }
  __syncthreads();
  if (tid == 0) mn.cnt[par ^ 1] = 0;   // the other set's counter: read last before this barrier, used next after the next
  int bw = 0;
#pragma unroll
  for (int w = 0; w < PL_WAVES; ++w) {
    const uint64_t w1 = mn.k1[par][w], w2 = mn.k2[par][w];
    th = w == 0 ? mn.th[par][w] : min(th, mn.th[par][w]);
    if (w == 0) {
      a1 = w1;
      a2 = w2;
    } else {
      const uint64_t m2 = min(a2, w2);
      if (w1 < a1) {
        a2 = min(a1, m2);
        a1 = w1;
        bw = w;
      } else {
        a2 = min(w1, m2);
      }
    }
  }
  bw = __builtin_amdgcn_readfirstlane(bw);
  LeastChoice c;   // the same on every thread; said so for the branches and barriers that follow
  c.k1 = uniform_u64(a1);
  c.k2 = uniform_u64(a2);
  c.th = uniform_u64(th);
  c.at = __builtin_amdgcn_readfirstlane(mn.at[par][bw]);
  c.r0 = c.r1 = c.r2 = c.r3 = 0;
  if (!c.none()) {
    c.r0 = (int64_t)uniform_u64((uint64_t)mn.r[par][bw][0]);
    c.r1 = (int64_t)uniform_u64((uint64_t)mn.r[par][bw][1]);
    c.r2 = (int64_t)uniform_u64((uint64_t)mn.r[par][bw][2]);
    c.r3 = (int64_t)uniform_u64((uint64_t)mn.r[par][bw][3]);
  }
  return c;
}

// A run's length: the pods the argmin node (residuals c.r, key c.k1 < c.k2) takes of `left` pods of request s
// before another node is due -- the first i at which its key after i pods is no longer below k2, at most what it
// holds.  The node fits s, so its labels need no second look.  Called by whole waves; the same on every lane.
__device__ __forceinline__ uint32_t least_run_len(const LeastChoice& c, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                                  uint32_t need, uint32_t left) {
  const uint32_t tmax = take_of(c.r0, c.r1, c.r2, c.r3, s0, s1, s2, s3, left);   // >= 1
  if (c.k2 == NO_KEY) return tmax;   // the only node that fits
  const uint64_t g = c.k1 & 0xFFFFFFu;
  const int64_t lane1 = (threadIdx.x & 63) + 1;
  int64_t lo = 1, hi = tmax;   // the answer lies in [lo, hi]; the key after lo - 1 pods is below k2
  while (lo < hi) {
    const int64_t step = (hi - lo) / 64 + 1;
    const int64_t x = lo - 1 + step * lane1;   // the lanes' probes ascend; x < hi <= take_of: x * s_d <= r_d
    bool below = false;
    if (x < hi)
      below = least_key(c.r0 - x * s0, c.r1 - x * s1, c.r2 - x * s2, c.r3 - x * s3, need, s0, s1, s2, s3, need, g) < c.k2;
    const int64_t yes = __popcll(__ballot(below));   // a prefix of the lanes: the key does not fall as x grows
    hi = min(hi, lo - 1 + step * (yes + 1));         // the first probe that was not below, if it was made
    lo += step * yes;
  }
  return (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)lo);
}

// A round: the members of W = { key < c.th } append their keys to list (cnt[par]: zero on entry), and the
// min(|W|, left) with the smallest keys take one pod of request s each off their own places.  Returns the pods
// placed, the same on every thread; 0 (CAPPED only): more than LS_RANK_MAX members, nothing taken -- the caller
// makes the decision as a run.  on_win(place, rank, node id) follows every take, on the owner's thread.  list holds
// n keys.  Called by the whole workgroup.
template <bool CAPPED, class OnWin>
__device__ __forceinline__ uint32_t least_round(int64_t* r0, int64_t* r1, int64_t* r2, int64_t* r3, const uint32_t* gid,
                                                const uint32_t* lab, int n, int64_t s0, int64_t s1, int64_t s2,
                                                int64_t s3, uint32_t need, const LeastChoice& c, uint32_t left,
                                                uint64_t* list, LeastMin& mn, int par, OnWin&& on_win) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += PL_THREADS) {
    const uint64_t k = least_key(r0[i], r1[i], r2[i], r3[i], lab[i], s0, s1, s2, s3, need, gid[i]);
    if (k < c.th) list[atomicAdd(&mn.cnt[par], 1u)] = k;   // at most one entry per place: below n
  }
  __syncthreads();
  const uint32_t m = __builtin_amdgcn_readfirstlane(mn.cnt[par]);   // >= 2: k1 and k2 are below theta
  if (CAPPED && m > LS_RANK_MAX) return 0;
  const uint32_t take = min(m, left);
  for (int i = tid; i < n; i += PL_THREADS) {
    const int64_t x0 = r0[i], x1 = r1[i], x2 = r2[i], x3 = r3[i];
    const uint32_t g = gid[i];
    const uint64_t k = least_key(x0, x1, x2, x3, lab[i], s0, s1, s2, s3, need, g);
    if (k >= c.th) continue;
    uint32_t rank = 0;   // the keys are unique: every member has its own rank
    for (uint32_t e = 0; e < m && rank < take; ++e) rank += list[e] < k;
    if (rank >= take) continue;
    r0[i] = x0 - s0;
    r1[i] = x1 - s1;
    r2[i] = x2 - s2;
    r3[i] = x3 - s3;
    on_win(i, rank, g);
  }
  return take;
}

}  // namespace pe
