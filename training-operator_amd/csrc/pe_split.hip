// pe_gang_split_tree's descent (include/placement.h): the gang of a pick, selected into one domain of one
// level by tree_select_kernel (pe_tree.hip), spread over the fewest domains of every level below, down to
// (leaf, pods) parts.  Runs after the selection on the same device tables, picks and answers.
//
// tree_split_kernel: one wave (a block of 64 threads) per pick.  The lists S_l and S_{l-1} of (domain, pods)
// ping-pong in LDS, a third list takes a parent's whole parts before they are ordered: 3 * max_parts * 8 B of
// dynamic LDS, 24 KiB at PE_MAX_SPLIT_PARTS.  Per (parent, allotment a) of S_l the lanes stride over the
// parent's child list (the plan's CSR, ascending ids) in the threshold form of the rule (pe_split_plan.h):
//   1. the largest child value mx; v* = mx when mx >= a, else the largest v in [1, mx] with H(v) >= a by
//      bisection (H is a step function that changes only at child values, so that v is one) -- at most 31
//      passes, since mx < a < 2^31;
//   2. G and the number of children above v*, and from them t and r (split_tr);
//   3. one pass in id order: a ballot numbers the children equal to v*, the children above v* and the first t
//      equal ones are compacted into the third list, every other child with slots >= r competes for the last
//      part by (slots, id);
//   4. each whole part's place in the walk order is its rank by (slots descending, id ascending) among the
//      whole parts of its parent.
// With a fan-in of 64 at most every lane keeps its one child in registers and no pass touches memory again.
// Integers only; every choice is made by (slots, id), none by lane.  A list that would pass max_parts ends the
// pick as PE_SPLIT_TOO_MANY: lists never shrink on the way down.
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_split_plan.h"

namespace pe {

namespace {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// S_{l-1} (dst) from S_l (src, ns entries); row: the shape's slots of level l - 1, start / child: level l's CSR.
// Returns |S_{l-1}|, or -1 when it would pass max_parts.  Every lane takes every branch alike.
__device__ int split_level(const unsigned long long* __restrict__ row, const int32_t* __restrict__ start,
                           const int32_t* __restrict__ child, const int2* src, int2* dst, int2* tmp, int ns,
                           int max_parts, int lane) {
  int nd = 0;
  for (int i = 0; i < ns; ++i) {
    const int2 pa = src[i];
    const uint64_t a = (uint64_t)(uint32_t)pa.y;   // 1 <= a <= the parent's slots
    const int b = start[pa.x], n = start[pa.x + 1] - b;
    const int32_t* ch = child + b;
    const bool small = n <= 64;
    int32_t cid = -1;
    uint64_t xr = 0;
    if (small && lane < n) {
      cid = ch[lane];
      xr = row[cid];
    }
    uint64_t mx = xr;
    if (!small)
      for (int q = lane; q < n; q += 64) {
        const uint64_t x = row[ch[q]];
        mx = x > mx ? x : mx;
      }
    mx = wave_max_u64(mx);
    uint64_t v = mx;
    if (mx < a) {   // H(1) = the parent's slots >= a > mx: the values fit 31 bits
      uint64_t lo = 1, hi = mx;
      while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        uint64_t h = 0;
        if (small) {
          h = xr >= mid ? xr : 0;
        } else {
          for (int q = lane; q < n; q += 64) {
            const uint64_t x = row[ch[q]];
            h += x >= mid ? x : 0;
          }
        }
        if (wave_sum_u64(h) >= a) lo = mid; else hi = mid - 1;
      }
      v = lo;
    }
    uint64_t G = 0;
    uint32_t above = 0;
    if (small) {
      G = xr > v ? xr : 0;
      above = xr > v ? 1u : 0u;
    } else {
      for (int q = lane; q < n; q += 64) {
        const uint64_t x = row[ch[q]];
        G += x > v ? x : 0;
        above += x > v ? 1u : 0u;
      }
    }
    G = wave_sum_u64(G);
    above = (uint32_t)wave_sum_u64(above);
    if (v == 0 || G >= a) return -1;   // (a table that is no roll-up of its children: not reached)
    const SplitTR tr = split_tr(a, G, v);
    const uint64_t k64 = (uint64_t)above + tr.t;
    if ((uint64_t)nd + k64 + 1 > (uint64_t)max_parts) return -1;
    const uint32_t t = (uint32_t)tr.t;
    uint32_t eq_run = 0, wh_run = 0, bid = ~0u;
    uint64_t bx = ~uint64_t(0);
    for (int q0 = 0; q0 < n; q0 += 64) {
      const int q = q0 + lane;
      const bool valid = q < n;
      int32_t c = cid;
      uint64_t x = xr;
      if (!small) {
        c = valid ? ch[q] : -1;
        x = valid ? row[c] : 0;
      }
      const bool eq = valid && x == v;
      const uint64_t em = __builtin_amdgcn_ballot_w64(eq);
      const bool whole = valid && (x > v || (eq && eq_run + lanes_below(em) < t));
      const uint64_t wm = __builtin_amdgcn_ballot_w64(whole);
      if (whole) {   // in id order; a whole part's slots are below a
        const uint32_t pos = wh_run + lanes_below(wm);
        if (pos < (uint32_t)max_parts) tmp[pos] = make_int2(c, (int)x);
      }
      eq_run += (uint32_t)__builtin_popcountll(em);
      wh_run += (uint32_t)__builtin_popcountll(wm);
      if (valid && !whole && x >= tr.r && x < bx) {   // c ascends within a lane: the first of equal values stays
        bx = x;
        bid = (uint32_t)c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t ox = __shfl_xor(bx, o, 64);
      const uint32_t oi = __shfl_xor(bid, o, 64);
      if (ox < bx || (ox == bx && oi < bid)) {
        bx = ox;
        bid = oi;
      }
    }
    if (bid == ~0u || wh_run != (uint32_t)k64) return -1;   // (not reached, as above)
    const int k = (int)wh_run;
    __syncthreads();
    for (int e = lane; e < k; e += 64) {
      const int2 me = tmp[e];
      int rank = 0;
      for (int f = 0; f < k; ++f) {
        const int2 o = tmp[f];
        rank += (o.y > me.y || (o.y == me.y && o.x < me.x)) ? 1 : 0;
      }
      dst[nd + rank] = me;
    }
    if (lane == 0) dst[nd + k] = make_int2((int)bid, (int)tr.r);
    nd += k + 1;
    __syncthreads();
  }
  return nd;
}

__global__ __launch_bounds__(64) void tree_split_kernel(const unsigned long long* __restrict__ leaf_slots,
                                                        const unsigned long long* __restrict__ upper_slots, int s0,
                                                        int S, TreeLevels lv, SplitCsr csr,
                                                        const int32_t* __restrict__ plan,
                                                        const TreePick* __restrict__ picks,
                                                        const TreeSel* __restrict__ sel, int p0, int n, int max_parts,
                                                        int32_t* __restrict__ buf) {
  extern __shared__ int2 split_lds[];
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (k >= n) return;
  const TreePick pk = picks[p0 + k];
  const int64_t s = (int64_t)pk.shape - s0;
  if (s < 0 || s >= S) return;   // a row of another launch
  const TreeSel a = sel[p0 + k];
  int2* src = split_lds;
  int2* dst = split_lds + max_parts;
  int2* const tmp = split_lds + 2 * max_parts;
  int np = 0;
  int32_t spread[TR_MAX_LEVELS] = {0, 0, 0, 0};
  if (a.level >= 0) {
    if (lane == 0) src[0] = make_int2(a.domain, pk.count);
    np = 1;
    __syncthreads();
#pragma unroll
    for (int l = TR_MAX_LEVELS - 1; l >= 1; --l) {
      if (l > a.level || np < 0) continue;
      spread[l] = np;
      const unsigned long long* row =
          l == 1 ? leaf_slots + s * lv.size[0] : upper_slots + s * lv.pitch + lv.col[l - 1];
      np = split_level(row, plan + csr.start_at[l], plan + csr.child_at[l], src, dst, tmp, np, max_parts, lane);
      int2* const sw = src;
      src = dst;
      dst = sw;
    }
    spread[0] = np;
  }
  const bool many = np < 0;
  const SplitLayout L{n, max_parts};
  int32_t* const o_dom = buf + L.dom_at() + (int64_t)k * max_parts;
  int32_t* const o_pods = buf + L.pods_at() + (int64_t)k * max_parts;
  for (int i = lane; i < max_parts; i += 64) {   // the unused tail: -1 / 0
    const int2 e = i < np ? src[i] : make_int2(-1, 0);
    o_dom[i] = e.x;
    o_pods[i] = e.y;
  }
  if (lane == 0) {
    int32_t* const meta = buf + L.meta_at() + (int64_t)k * SPLIT_META_WORDS;
    meta[0] = many ? SPLIT_TOO_MANY : np;
#pragma unroll
    for (int l = 0; l < TR_MAX_LEVELS; ++l) meta[1 + l] = many ? 0 : spread[l];
  }
}

}  // namespace

hipError_t launch_tree_split(hipStream_t s, const uint64_t* leaf_slots, const uint64_t* upper_slots, int64_t s0,
                             int64_t S, const TreeLevels& levels, const SplitCsr& csr, const int32_t* plan,
                             const TreePick* picks, const TreeSel* sel, int64_t p0, int64_t n, int max_parts,
                             int32_t* buf) {
  if (n <= 0 || S <= 0) return hipSuccess;
  if (max_parts < 1 || max_parts > SPLIT_MAX_PARTS || n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const size_t lds = (size_t)3 * (size_t)max_parts * sizeof(int2);
  hipLaunchKernelGGL(tree_split_kernel, dim3((unsigned)n), dim3(64), lds, s, (const unsigned long long*)leaf_slots,
                     (const unsigned long long*)upper_slots, (int)s0, (int)S, levels, csr, plan, picks, sel, (int)p0,
                     (int)n, max_parts, buf);
  return hipGetLastError();
}

}  // namespace pe
