// The Appendix-B rule under a per-spread-domain pod cap (pe_place_spread_domains; device code only): one DECISION
// (spread_decide) and the WALK of a job's groups through it (spread_group, spread_groups), beside pe_place_step.h,
// whose key, take, argmin and choice they reuse and whose own decision stays as it is.
//
// The rule pod by pod: a pod of group g with cap m goes to the argmin-key node among the nodes that fit and whose
// spread domain holds fewer than m pods of g.  TAKE-MANY stays exact: after a pod lands on node n, n's leftover
// falls, so its score falls or stays saturated, and its id is the same -- n's key never rises, and no other node's
// key moves at all.  The cap can only remove candidates, and it removes n only once n's spread domain is full.  So
// n stays the argmin until it no longer fits or its spread domain is full, and one decision takes
//   t = min(take_of(n), allowance(sd(n)), pods left)
// pods, which is what t pod-by-pod steps would have done.  An island group is one unit of `count` pods: it needs a
// node that fits count x request and whose spread domain still allows count.
//
// The allowance is kept PER PLACE, two more words beside the working state:
//   allow[i]   what the spread domain of place i still allows the current group; set to the cap at group start
//   sub[i]     (spread domains above the node) which spread domain of the segment place i is in
// A decision's outcome -- the spread domain u = sub[c.at] it landed in and the pods t it took -- is the same on
// every thread, and it is applied LAZILY: it rides into the next decision's scoring pass, where every thread takes t
// off allow[i] of its own places with sub[i] == u before it scores them.  So thread i mod PL_THREADS stays the only
// one that reads or writes place i, a decision still costs one barrier, and no pass over the segment is added.  With
// the node as the spread domain the owner of the chosen place takes t off its one word as it takes the request.
// allow is 32 bits wide and exact: caps and counts reach 2^31 - 1, and a group takes at most its count off a word
// that started at a cap >= 1, so no word wraps.
#pragma once
#include "pe_place_step.h"

namespace pe {

// place_decide with the allowance in the fit: a place with allow 0 (unit: below `left`, the group's count) scores
// NO_KEY, and the take is cut to the allowance.  (pu, pt): the decision before this one of the same group took pt
// pods in spread domain pu; pt == 0: none.  Called by the whole workgroup.
template <bool BY_NODE>
__device__ __forceinline__ PlaceChoice spread_decide(const int64_t* r0, const int64_t* r1, const int64_t* r2,
                                                     const int64_t* r3, const uint32_t* gid, const uint32_t* lab,
                                                     uint32_t* allow, const uint32_t* sub, int n, int64_t s0, int64_t s1,
                                                     int64_t s2, int64_t s3, uint32_t need, bool unit, uint32_t left,
                                                     uint32_t pu, uint32_t pt, PlaceMin& mn, int& par) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t floor_ = unit ? left : 1u;   // the allowance a place needs to take part
  uint64_t bk = NO_KEY;
  uint32_t bi = 0, bt = 0, ba = 0;
  for (int i = tid; i < n; i += PL_THREADS) {
    uint32_t a = allow[i];
    if constexpr (!BY_NODE) {
      if (pt != 0 && sub[i] == pu) {
        a -= pt;   // >= 0: the take was cut to this very allowance
        allow[i] = a;
      }
    }
    const uint64_t k =
        a >= floor_ ? node_key(r0[i], r1[i], r2[i], r3[i], lab[i], s0, s1, s2, s3, need, gid[i]) : NO_KEY;
    if (k < bk) {
      bk = k;
      bi = (uint32_t)i;
      ba = a;
    }
  }
  if (bk != NO_KEY) bt = unit ? left : min(take_of(r0[bi], r1[bi], r2[bi], r3[bi], s0, s1, s2, s3, left), ba);
  wave_argmin_u64(bk, bi, bt);
  if (lane == 0) {
    mn.key[par][wave] = bk;
    mn.at[par][wave] = bi;
    mn.take[par][wave] = bt;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < PL_WAVES; ++w) {
    const uint64_t k = mn.key[par][w];
    if (w == 0 || k < bk) {
      bk = k;
      bi = mn.at[par][w];
      bt = mn.take[par][w];
    }
  }
  par ^= 1;
  PlaceChoice c;   // the same on every thread
  c.klo = __builtin_amdgcn_readfirstlane((uint32_t)bk);
  c.khi = __builtin_amdgcn_readfirstlane((uint32_t)(bk >> 32));
  c.at = __builtin_amdgcn_readfirstlane(bi);
  c.t = __builtin_amdgcn_readfirstlane(bt);
  return c;
}

// place_group under the cap `cap` (>= 1; SPREAD_UNCAPPED never binds): one group on the working state w0[d * ws + i]
// with allow[i] (written) and, !BY_NODE, sub[i] beside it, until its pods are placed or one finds no node; the pods
// left, the same on every thread.  on_take(c, done) follows every take.  Called by the whole workgroup.
template <bool BY_NODE, class Stride, class OnTake>
__device__ __forceinline__ uint32_t spread_group(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab,
                                                 uint32_t* allow, const uint32_t* sub, int n, PlaceMin& mn, int& par,
                                                 const PlaceGroup& gr, uint32_t cap, OnTake&& on_take) {
  if (gr.count <= 0) return 0;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  const bool unit = (gr.need & NEED_ISLAND) != 0;
  int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
  uint32_t left = (uint32_t)gr.count;
  if (unit && !island_request(gr, s0, s1, s2, s3)) return left;
  for (int i = threadIdx.x; i < n; i += PL_THREADS) allow[i] = cap;   // the owner's places: no barrier
  uint32_t pu = 0, pt = 0;
  while (left > 0) {
    const PlaceChoice c =
        spread_decide<BY_NODE>(w0, w1, w2, w3, gid, lab, allow, sub, n, s0, s1, s2, s3, gr.need, unit, left, pu, pt, mn, par);
    if (c.none()) break;   // no node of the domain fits under the cap
    place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3);
    if constexpr (BY_NODE) {
      if ((c.at & (PL_THREADS - 1)) == threadIdx.x) allow[c.at] -= c.t;
    } else {
      pu = sub[c.at];   // read-only since the segment was staged, and a barrier lies between
      pt = c.t;
    }
    on_take(c, (uint32_t)gr.count - left);
    left -= c.t;
  }
  return left;
}

// place_groups with the groups' caps: groups [g0, g1) in order, stopping at the first that is not placed in full.
template <bool BY_NODE, class Stride, class OnTake>
__device__ __forceinline__ int spread_groups(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab,
                                             uint32_t* allow, const uint32_t* sub, int n, PlaceMin& mn, int& par,
                                             const PlaceGroup* __restrict__ groups, const int32_t* __restrict__ caps, int g0,
                                             int g1, uint32_t& left, OnTake&& on_take) {
  left = 0;
  int g = g0;
  while (g < g1 && left == 0) {
    const PlaceGroup gr = groups[g];
    const uint32_t cap = (uint32_t)caps[g];
    left = spread_group<BY_NODE>(w0, ws, gid, lab, allow, sub, n, mn, par, gr, cap,
                                 [&](const PlaceChoice& c, uint32_t done) { on_take(g, gr, c, done); });
    g += 1 - (int)min(left, 1u);
  }
  return g;
}

}  // namespace pe
