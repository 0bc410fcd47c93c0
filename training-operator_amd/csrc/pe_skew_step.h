// The Appendix-B rule under maxSkew (pe_place_skew_domains; device code only): one DECISION (skew_decide), the uniform
// SKEW STATE it reads (SkewState, skew_open, skew_scan) and the WALK of a job's groups through it (skew_group,
// skew_groups), beside pe_place_step.h, whose key, take, island request and place_take they reuse, and whose own
// walk serves the unconstrained groups as it is.
//
// The rule pod by pod, for a group with maxSkew s: cnt[u] = the pods the constraint counts in spread domain u (the
// caller's book plus this group's pods from this call), gmin = the minimum of cnt over the ELIGIBLE spread domains
// (those with a node of the segment whose labels match, full or not); a pod goes to the argmin-key node among the
// fitting nodes n with cnt[sd(n)] + 1 - gmin <= s.
//
// gmin moves while pods are placed, and when it rises places come IN: pe_spread_step.h's "candidates only go away"
// does not hold.  What replaces it is three uniform numbers,
//   m1   the smallest count,   n1   how many eligible spread domains hold it,   m2   the smallest count above m1
// (SK_OUT: none).  For a spread domain u with count c the minimum over the OTHER eligible domains is
//   m_other(u) = (c == m1 && n1 == 1) ? m2 : m1        (SK_OUT: there is no other one, nothing bounds u)
// and u can take A(u) = s + m_other(u) - c more pods in a row: while u is the only minimum every pod raises gmin
// with it, and from m2 on gmin stands.  A place takes part iff it fits and A >= 1 (an island unit: >= count), which
// is the pod-by-pod predicate.  TAKE-MANY, for the argmin u* under the skew:
//   - u* is not the only minimum: gmin cannot move during the run, candidates only go away, and only once u* is full:
//     t = min(take_of, A(u*), left), as under a cap;
//   - u* is the only minimum: each pod raises gmin and may admit places of other domains.  If the chosen place is
//     also the argmin over ALL fitting places, nothing admitted can beat it (its key only falls, no other key
//     moves): the same t, with A on m2.  Otherwise one pod, and the next decision sees who came in.
// Both argmins come out of one block reduction, so a decision costs one barrier.
//
// The counts are kept PER PLACE, as pe_spread_step.h keeps its allowance: cnt[i] is the count of place i's spread
// domain and sub[i] the domain's FIRST place in the segment (its representative; the place itself when the spread
// domain is the node).  A decision's outcome (u*, t) is the same on every thread and rides into the next scoring
// pass, where every thread adds t to its own places of u* before it scores them: thread i mod PL_THREADS stays the
// only one that reads or writes place i between group starts.  (m1, n1, m2) follow every take by arithmetic; they
// are counted again over the representatives (skew_scan: one pass, one barrier more) only when the only minimum
// reached m2 -- then how many domains stand at the new minimum is not known -- or when the value m2 named was taken
// away and an only minimum needs it.  Counts are 32 bits wide and exact: a book entry and a group's pods are below
// 2^31 each, so no sum reaches SK_OUT.
#pragma once
#include "pe_place_step.h"

namespace pe {

constexpr uint32_t SK_OUT = 0xFFFFFFFFu;   // cnt of a place whose spread domain is not eligible; m2: no such count

struct SkewMin {   // the waves' slots: the family's, the decision's two sets and the scan's
  PlaceMin pm;
  uint64_t key[2][PL_WAVES], all[2][PL_WAVES];
  uint32_t at[2][PL_WAVES], take[2][PL_WAVES], c0[2][PL_WAVES];
  uint32_t m1[PL_WAVES], n1[PL_WAVES], m2[PL_WAVES];
};
struct SkewState {
  uint32_t m1, n1, m2;
  bool stale;   // m2 may name a count that no domain holds any more: a lower bound, read only after a scan
};
// What a group's walk needs beside the working state: the rows, the segment's first place b, what sub's values
// are relative to (sb: b where the row is the scratch row, 0 where it was staged), the book and the key -> place row.
struct SkewRows {
  uint32_t* cnt;
  const uint32_t* sub;
  uint32_t b, sb;
  const int32_t* __restrict__ skew;
  const int32_t* __restrict__ book_off;
  const int32_t* __restrict__ book;   // [E][2]: an entry's key and the pods its spread domain already holds
  const int32_t* __restrict__ where;   // [n_keys]
  uint32_t n_keys, id_base;
};

// (m1, n1, m2) of two sets of counts from theirs.  The empty set is (SK_OUT, 0, SK_OUT).
__device__ __forceinline__ void skew_fold(uint32_t& m1, uint32_t& n1, uint32_t& m2, uint32_t o1, uint32_t on, uint32_t o2) {
  if (o1 == m1) {
    n1 += on;
    m2 = min(m2, o2);
  } else if (o1 < m1) {
    m2 = min(o2, m1);
    m1 = o1;
    n1 = on;
  } else {
    m2 = min(m2, o1);
  }
}

// The state counted over the representatives, after the pending take (pu, pt; pt == 0: none) went onto the threads'
// own places.  Called by the whole workgroup; one barrier.
__device__ __forceinline__ SkewState skew_scan(const SkewRows& rw, int n, uint32_t pu, uint32_t pt, SkewMin& mn) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t m1 = SK_OUT, n1 = 0, m2 = SK_OUT;
  for (int i = tid; i < n; i += PL_THREADS) {
    const uint32_t u = rw.sub[i] - rw.sb;
    uint32_t c = rw.cnt[i];
    if (pt != 0 && u == pu) {
      c += pt;
      rw.cnt[i] = c;
    }
    if (u == (uint32_t)i && c != SK_OUT) skew_fold(m1, n1, m2, c, 1u, SK_OUT);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t o1 = __shfl_xor(m1, o, 64), on = __shfl_xor(n1, o, 64), o2 = __shfl_xor(m2, o, 64);
    skew_fold(m1, n1, m2, o1, on, o2);
  }
  if (lane == 0) {
    mn.m1[wave] = m1;
    mn.n1[wave] = n1;
    mn.m2[wave] = m2;
  }
  __syncthreads();
  m1 = mn.m1[0], n1 = mn.n1[0], m2 = mn.m2[0];
#pragma unroll
  for (int w = 1; w < PL_WAVES; ++w) skew_fold(m1, n1, m2, mn.m1[w], mn.n1[w], mn.m2[w]);
  SkewState st;   // the same on every thread
  st.m1 = __builtin_amdgcn_readfirstlane(m1);
  st.n1 = __builtin_amdgcn_readfirstlane(n1);
  st.m2 = __builtin_amdgcn_readfirstlane(m2);
  st.stale = false;
  return st;
}

// A constrained group's start: cnt of every place from the labels (`need`) and the group's book entries [e0, e1),
// and the state.  The representative's word is where a spread domain's places meet: the owners mark it, the book's
// entries land on it (keys are unique within a group: no two writers), the owners copy it.  Four barriers, once per
// group; a rollback never touches the counts, they are rebuilt here.  Called by the whole workgroup.
__device__ __forceinline__ SkewState skew_open(const SkewRows& rw, const uint32_t* lab, int n, uint32_t need, int e0,
                                               int e1, SkewMin& mn) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += PL_THREADS) rw.cnt[i] = SK_OUT;
  __syncthreads();
  for (int i = tid; i < n; i += PL_THREADS) {
    const uint32_t u = rw.sub[i] - rw.sb;   // a place of this segment: a spread domain lies in one domain of the level
    if (u < (uint32_t)n && (lab[i] & need) == need) rw.cnt[u] = 0;   // every writer writes 0
  }
  __syncthreads();
  for (int e = e0 + tid; e < e1; e += PL_THREADS) {
    const uint32_t key = (uint32_t)rw.book[2 * e] - rw.id_base;
    if (key >= rw.n_keys) continue;                        // the plan checked the entry
    const uint32_t at = (uint32_t)rw.where[key] - rw.b;   // the key's first place; none: INT32_MAX
    if (at < (uint32_t)n && rw.cnt[at] != SK_OUT) rw.cnt[at] = (uint32_t)rw.book[2 * e + 1];   // else: not under this domain
  }
  __syncthreads();
  for (int i = tid; i < n; i += PL_THREADS) {
    const uint32_t u = rw.sub[i] - rw.sb;
    if (u != (uint32_t)i && u < (uint32_t)n) rw.cnt[i] = rw.cnt[u];   // reads representatives, writes the others
  }
  return skew_scan(rw, n, 0, 0, mn);
}

// The block's choice under the skew: place_decide with A in the fit and in the take.  c0: the count of the chosen
// place's spread domain before the take.  (pu, pt): the decision before this one of the same group took pt pods in
// the spread domain whose representative is pu; pt == 0: none.  Called by the whole workgroup; one barrier.
struct SkewChoice {
  PlaceChoice c;
  uint32_t c0;
};
__device__ __forceinline__ SkewChoice skew_decide(const int64_t* r0, const int64_t* r1, const int64_t* r2,
                                                  const int64_t* r3, const uint32_t* gid, const uint32_t* lab,
                                                  const SkewRows& rw, int n, int64_t s0, int64_t s1, int64_t s2,
                                                  int64_t s3, uint32_t need, bool unit, uint32_t left, uint32_t skew,
                                                  uint32_t pu, uint32_t pt, const SkewState& st, SkewMin& mn, int& par) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t floor_ = unit ? left : 1u;   // the pods in a row a place must be allowed to take part
  uint64_t bk = NO_KEY, ka = NO_KEY;
  uint32_t bi = 0, bt = 0, bc = 0, ba = 0;
  for (int i = tid; i < n; i += PL_THREADS) {
    uint32_t c = rw.cnt[i];
    if (pt != 0 && rw.sub[i] - rw.sb == pu) {
      c += pt;
      rw.cnt[i] = c;
    }
    const uint64_t k = node_key(r0[i], r1[i], r2[i], r3[i], lab[i], s0, s1, s2, s3, need, gid[i]);
    ka = min(ka, k);
    const uint32_t mo = (c == st.m1 && st.n1 == 1u) ? st.m2 : st.m1;
    // A = skew + mo - c; a fitting place is in an eligible domain: c != SK_OUT, and mo <= c unless it is m2
    const int64_t A = mo == SK_OUT ? (int64_t)0xFFFFFFFF : (int64_t)skew + (int64_t)mo - (int64_t)c;
    if (k < bk && A >= (int64_t)floor_) {
      bk = k;
      bi = (uint32_t)i;
      bc = c;
      ba = (uint32_t)min(A, (int64_t)0xFFFFFFFF);
    }
  }
  if (bk != NO_KEY) bt = unit ? left : min(take_of(r0[bi], r1[bi], r2[bi], r3[bi], s0, s1, s2, s3, left), ba);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t ok = __shfl_xor(bk, o, 64);
    const uint32_t oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64), oc = __shfl_xor(bc, o, 64);
    ka = min(ka, (uint64_t)__shfl_xor(ka, o, 64));
    if (ok < bk) {
      bk = ok;
      bi = oi;
      bt = ot;
      bc = oc;
    }
  }
  if (lane == 0) {
    mn.key[par][wave] = bk;
    mn.all[par][wave] = ka;
    mn.at[par][wave] = bi;
    mn.take[par][wave] = bt;
    mn.c0[par][wave] = bc;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < PL_WAVES; ++w) {
    const uint64_t k = mn.key[par][w];
    ka = w == 0 ? mn.all[par][0] : min(ka, mn.all[par][w]);
    if (w == 0 || k < bk) {
      bk = k;
      bi = mn.at[par][w];
      bt = mn.take[par][w];
      bc = mn.c0[par][w];
    }
  }
  par ^= 1;
  // the only minimum, and some place the skew keeps out scores better: one pod, then look again
  if (!unit && bc == st.m1 && st.n1 == 1u && ka != bk) bt = min(bt, 1u);
  SkewChoice ch;   // the same on every thread
  ch.c.klo = __builtin_amdgcn_readfirstlane((uint32_t)bk);
  ch.c.khi = __builtin_amdgcn_readfirstlane((uint32_t)(bk >> 32));
  ch.c.at = __builtin_amdgcn_readfirstlane(bi);
  ch.c.t = __builtin_amdgcn_readfirstlane(bt);
  ch.c0 = __builtin_amdgcn_readfirstlane(bc);
  return ch;
}

// place_group under maxSkew `skew` (>= 1) with the group's book entries [e0, e1): one group on the working state
// w0[d * ws + i] until its pods are placed or one finds no node; the pods left, the same on every thread.
// on_take(c, done) follows every take.  Called by the whole workgroup.
template <class Stride, class OnTake>
__device__ __forceinline__ uint32_t skew_group(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab,
                                               const SkewRows& rw, int n, SkewMin& mn, int& par, const PlaceGroup& gr,
                                               uint32_t skew, int e0, int e1, OnTake&& on_take) {
  if (gr.count <= 0) return 0;
  int64_t* const w1 = w0 + ws;
  int64_t* const w2 = w1 + ws;
  int64_t* const w3 = w2 + ws;
  const bool unit = (gr.need & NEED_ISLAND) != 0;
  int64_t s0 = gr.q[0], s1 = gr.q[1], s2 = gr.q[2], s3 = gr.q[3];
  uint32_t left = (uint32_t)gr.count;
  if (unit && !island_request(gr, s0, s1, s2, s3)) return left;
  SkewState st = skew_open(rw, lab, n, gr.need, e0, e1, mn);
  uint32_t pu = 0, pt = 0;
  bool again = false;   // the state is to be counted again before the next decision
  while (left > 0) {
    if (again || (st.stale && st.n1 == 1u)) {
      st = skew_scan(rw, n, pu, pt, mn);
      pt = 0;
      again = false;
    }
    const SkewChoice ch =
        skew_decide(w0, w1, w2, w3, gid, lab, rw, n, s0, s1, s2, s3, gr.need, unit, left, skew, pu, pt, st, mn, par);
    const PlaceChoice& c = ch.c;
    if (c.none()) break;   // no node of the domain fits under the skew
    place_take(w0, w1, w2, w3, c, unit, s0, s1, s2, s3);
    const uint32_t c1 = ch.c0 + c.t;
    if (ch.c0 == st.m1) {
      if (st.n1 > 1u) {   // one of several minima moved up
        --st.n1;
        st.m2 = min(st.m2, c1);
      } else if (c1 < st.m2) {   // the only minimum, still below the next count
        st.m1 = c1;
      } else {
        again = true;
      }
    } else if (ch.c0 == st.m2) {
      st.stale = true;
    }
    pu = rw.sub[c.at] - rw.sb;   // read-only since the segment was staged, and a barrier lies between
    pt = c.t;
    on_take(c, (uint32_t)gr.count - left);
    left -= c.t;
  }
  return left;
}

// place_groups with the groups' skews: groups [g0, g1) in order, stopping at the first that is not placed in full.
// A group without a constraint (skew 0) walks through place_group itself.
template <class Stride, class OnTake>
__device__ __forceinline__ int skew_groups(int64_t* w0, Stride ws, const uint32_t* gid, const uint32_t* lab,
                                           const SkewRows& rw, int n, SkewMin& mn, int& par,
                                           const PlaceGroup* __restrict__ groups, int g0, int g1, uint32_t& left,
                                           OnTake&& on_take) {
  left = 0;
  int g = g0;
  while (g < g1 && left == 0) {
    const PlaceGroup gr = groups[g];
    const uint32_t skew = (uint32_t)rw.skew[g];
    const auto took = [&](const PlaceChoice& c, uint32_t done) { on_take(g, gr, c, done); };
    left = skew == 0u ? place_group(w0, ws, gid, lab, n, mn.pm, par, gr, took)
                      : skew_group(w0, ws, gid, lab, rw, n, mn, par, gr, skew, rw.book_off[g], rw.book_off[g + 1], took);
    g += 1 - (int)min(left, 1u);
  }
  return g;
}

}  // namespace pe
