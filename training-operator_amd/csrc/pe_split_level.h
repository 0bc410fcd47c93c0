// One level of the descent of pe_gang_split_tree (pe_split.hip states the step) for one wave: S_{l-1} from S_l.
// Shared with pe_gang_slice_tree's descent (pe_slice.hip), whose lists hold units above the slice level and pods
// below it: the step is the same in either.
#pragma once
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

}  // namespace

}  // namespace pe
