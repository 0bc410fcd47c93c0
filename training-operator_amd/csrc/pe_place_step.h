// The Appendix-B rule inside a domain's segment, stated once for every domain call (device code only): one
// DECISION (place_decide, place_take) and the WALK of a job's groups through it (place_group, place_groups), the
// only place where the island test, island_request, the loop over the pods left, none() and place_take are strung
// together.  The placing kernels (pe_place_job.h: place_job; pe_place_min.hip: place_optional) and the what-if
// kernels (pe_fit.hip, pe_preempt.hip, pe_drain.hip, pe_scale.hip, framed by pe_what_if.h) are callers that say what
// happens after a take.
// Per decision every thread scores its share of the segment with node_key (pe_node_key.h) against the working
// residuals and finds what its own best node would take; a wave butterfly (pe_wave.h) and one cross-wave step
// through LDS give the block's minimum key with that node's place and take.  Thread i mod PL_THREADS is the only
// one that reads or writes place i of the working state, so a decision costs one barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pe_kernels.h"
#include "pe_node_key.h"
#include "pe_wave.h"

namespace pe {

constexpr int PL_WAVES = PL_THREADS / 64;
constexpr uint32_t NEED_ISLAND = 0x80000000u;   // PE_NEED_ISLAND

// What node state (r0 .. r3) takes of `left` pods of request q: min(left, min over q_d > 0 of floor(r_d / q_d)).
// Called for a node that fits one pod, so every r_d >= q_d >= 0.
__device__ __forceinline__ uint32_t take_of(int64_t r0, int64_t r1, int64_t r2, int64_t r3, int64_t q0, int64_t q1,
                                            int64_t q2, int64_t q3, uint32_t left) {
  uint64_t t = left;
  if (q0 > 0) t = min(t, (uint64_t)r0 / (uint64_t)q0);
  if (q1 > 0) t = min(t, (uint64_t)r1 / (uint64_t)q1);
  if (q2 > 0) t = min(t, (uint64_t)r2 / (uint64_t)q2);
  if (q3 > 0) t = min(t, (uint64_t)r3 / (uint64_t)q3);
  return (uint32_t)t;
}

struct PlaceShared {   // the global segment's shape with a stride of PL_LDS_NODES
  int64_t r[D][PL_LDS_NODES];
  uint32_t gid[PL_LDS_NODES];
  uint32_t lab[PL_LDS_NODES];
};
struct PlaceMin {   // the waves' minima of a decision, two sets used in turn: one barrier per decision
  uint64_t key[2][PL_WAVES];
  uint32_t at[2][PL_WAVES];
  uint32_t take[2][PL_WAVES];
};

// A SECOND SPAN of places beside the working state's n: places that are in no segment (pe_scale.hip: nodes that
// would join the domain).  Thread j holds place j of the span in its own registers -- x0 .. x3, its labels and its
// id, `live` where it has one -- so the span has at most PL_THREADS places, takes no LDS and thread j mod
// PL_THREADS stays the only one that touches its place j.  The block's choice names place j of the span as n + j.
// NoSpan, the default of everything below, is no span at all: the callers that pass none compile to what they
// were.
struct NoSpan {
  static constexpr bool present = false;
};
template <class Span>
constexpr bool has_span = std::remove_reference_t<Span>::present;

// An island group's request: count x request, the scan's request for its one decision.  False when a product
// overflows int64: the group fits nowhere.
__device__ __forceinline__ bool island_request(const PlaceGroup& gr, int64_t& s0, int64_t& s1, int64_t& s2, int64_t& s3) {
  bool ovf = __builtin_mul_overflow(gr.q[0], (int64_t)gr.count, &s0);
  ovf |= __builtin_mul_overflow(gr.q[1], (int64_t)gr.count, &s1);
  ovf |= __builtin_mul_overflow(gr.q[2], (int64_t)gr.count, &s2);
  ovf |= __builtin_mul_overflow(gr.q[3], (int64_t)gr.count, &s3);
  return !ovf;
}

// The block's choice for `left` pods of request s (unit: an island group, one decision for all of them) among
// the n places of the working state r0 .. r3 with ids gid and labels lab: the minimum key's halves, its place
// and its take, the same on every thread.  NO_KEY (klo & khi == ~0): no node of the segment fits.  Called by
// the whole workgroup; `par` alternates the two sets of `mn`.
struct PlaceChoice {
  uint32_t klo, khi, at, t;
  __device__ __forceinline__ bool none() const { return (klo & khi) == 0xFFFFFFFFu; }
};
template <class Span = NoSpan>
__device__ __forceinline__ PlaceChoice place_decide(const int64_t* r0, const int64_t* r1, const int64_t* r2,
                                                    const int64_t* r3, const uint32_t* gid, const uint32_t* lab, int n,
                                                    int64_t s0, int64_t s1, int64_t s2, int64_t s3, uint32_t need,
                                                    bool unit, uint32_t left, PlaceMin& mn, int& par,
                                                    Span&& span = Span()) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t bk = NO_KEY;
  uint32_t bi = 0, bt = 0;
  for (int i = tid; i < n; i += PL_THREADS) {
    const uint64_t k = node_key(r0[i], r1[i], r2[i], r3[i], lab[i], s0, s1, s2, s3, need, gid[i]);
    if (k < bk) {
      bk = k;
      bi = (uint32_t)i;
    }
  }
  bool own = false;   // the thread's best is its place of the second span
  if constexpr (has_span<Span>) {   // scored like every other place
    if (span.live) {
      const uint64_t k = node_key(span.x0, span.x1, span.x2, span.x3, span.lab, s0, s1, s2, s3, need, span.gid);
      if (k < bk) {
        bk = k;
        bi = (uint32_t)(n + tid);
        own = true;
        bt = unit ? left : take_of(span.x0, span.x1, span.x2, span.x3, s0, s1, s2, s3, left);
      }
    }
  }
  if (!own && bk != NO_KEY) bt = unit ? left : take_of(r0[bi], r1[bi], r2[bi], r3[bi], s0, s1, s2, s3, left);
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
  // the same on every thread; said so for the branches and barriers that follow
  PlaceChoice c;
  c.klo = __builtin_amdgcn_readfirstlane((uint32_t)bk);
  c.khi = __builtin_amdgcn_readfirstlane((uint32_t)(bk >> 32));
  c.at = __builtin_amdgcn_readfirstlane(bi);
  c.t = __builtin_amdgcn_readfirstlane(bt);
  return c;
}

// The chosen place's owner takes the choice off the working state: t pods of request s, or the island group's
// one unit (s = count x request, t = count).  t * s_d <= r_d.  A choice at n or beyond is place c.at - n of the
// second span, and comes off its owner's registers.
template <class Span = NoSpan>
__device__ __forceinline__ void place_take(int64_t* r0, int64_t* r1, int64_t* r2, int64_t* r3, const PlaceChoice& c,
                                           bool unit, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int n = 0,
                                           Span&& span = Span()) {
  if constexpr (has_span<Span>) {
    if (c.at >= (uint32_t)n) {
      if (c.at - (uint32_t)n != threadIdx.x) return;
      const int64_t m = unit ? 1 : (int64_t)c.t;
      span.x0 -= m * s0;
      span.x1 -= m * s1;
      span.x2 -= m * s2;
      span.x3 -= m * s3;
      return;
    }
  }
  if ((c.at & (PL_THREADS - 1)) != threadIdx.x) return;
  const int64_t m = unit ? 1 : (int64_t)c.t;
  r0[c.at] -= m * s0;
  r1[c.at] -= m * s1;
  r2[c.at] -= m * s2;
  r3[c.at] -= m * s3;
}

// One group on the working state w0[d * ws + i] (written) of n places with ids gid and labels lab, until its pods
// are placed or one finds no node: the pods left (0: placed in full, or count <= 0), the same on every thread.  An
// island group is one decision for count x request, and a product that overflows fits nowhere.
// on_take(c, done) follows every take; done: the group's pods placed before it.  Called by the whole workgroup.
template <class Stride, class OnTake, class Span = NoSpan>
__device__ __forceinline__ uint32_t place_group(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab, int n,
                                                PlaceMin& mn, int& par, const PlaceGroup& gr, OnTake&& on_take,
                                                Span&& span = Span()) {
  if (gr.count <= 0) return 0;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  const bool unit = (gr.need & NEED_ISLAND) != 0;
  int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];   // the request the scan scores
  uint32_t left = (uint32_t)gr.count;
  if (unit && !island_request(gr, s0, s1, s2, s3)) return left;
  while (left > 0) {
    const PlaceChoice c = place_decide(w0, w1, w2, w3, gid, lab, n, s0, s1, s2, s3, gr.need, unit, left, mn, par, span);
    if (c.none()) break;   // no node of the domain fits
    place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3, n, span);
    on_take(c, (uint32_t)gr.count - left);
    left -= c.t;
  }
  return left;
}

// Groups [g0, g1) in order, stopping at the first that is not placed in full: that group (g1: all placed) and, in
// `left`, its pods left.  on_take(g, gr, c, done) as place_group's, with the group's index and record.
template <class Stride, class OnTake, class Span = NoSpan>
__device__ __forceinline__ int place_groups(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab, int n,
                                            PlaceMin& mn, int& par, const PlaceGroup* __restrict__ groups, int g0, int g1,
                                            uint32_t& left, OnTake&& on_take, Span&& span = Span()) {
  left = 0;
  int g = g0;
  while (g < g1 && left == 0) {
    const PlaceGroup gr = groups[g];
    left = place_group(w0, ws, gid, lab, n, mn, par, gr,
                       [&](const PlaceChoice& c, uint32_t done) { on_take(g, gr, c, done); }, span);
    g += 1 - (int)min(left, 1u);   // past a group placed in full (g += left == 0 took the flag through a VGPR)
  }
  return g;
}

}  // namespace pe
