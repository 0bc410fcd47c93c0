// The body of gang_capacity_domains_kernel (pe_domains.hip states it step by step), shared with the leaf kernel of
// pe_gang_slice_tree (pe_slice.hip).  SLICE: a shape record whose pad_[0] holds a slice size z >= 2 counts every
// node in whole slices, floor(cap / z), and only with at least one; pad_[0] == 0 leaves the record's row in slots.
// The division is wave-uniform in z.  Without SLICE the body is the domain kernel's, instruction for instruction.
#pragma once
#include <hip/hip_runtime.h>

#include "pe_capacity_eval.h"
#include "pe_kernels.h"
#include "pe_slice_plan.h"
#include "pe_wave.h"

namespace pe {

namespace {

constexpr int DM_HASH = 2 * CP_SPAN;       // dictionary keys: load factor <= 1/2
constexpr int DM_HASH_BITS = 11;
static_assert(DM_HASH == 1 << DM_HASH_BITS, "DM_HASH_BITS");
constexpr int DM_ACC = 4096;               // u64 accumulators per block (32 KiB)
static_assert(DM_ACC >= CP_SPAN, "a block with CP_SPAN distinct domains must hold one shape");
constexpr uint32_t DM_EMPTY = 0xFFFFFFFFu;   // no domain id: ids are below DM_MAX_DOMAINS
constexpr int DM_CNT_SHIFT = 48;
constexpr uint64_t DM_SUM_MASK = (uint64_t(1) << DM_CNT_SHIFT) - 1;
static_assert((uint64_t)CP_SPAN * CP_CAP_MAX <= DM_SUM_MASK, "a block's sum must stay below the packed count");

// The largest power of two w such that every aligned group of w lanes holds one value of x.  Called by
// the whole wave.
__device__ __forceinline__ int uniform_width(int x) {
  int w = 1;
  for (int o = 1; o < 64; o <<= 1) {
    const int other = __shfl_xor(x, o, 64);
    if (__builtin_amdgcn_ballot_w64(other != x) != 0) break;
    w <<= 1;
  }
  return w;
}

template <bool SLICE>
__device__ __forceinline__ void gang_capacity_domains_body(
    const int64_t* __restrict__ res, int64_t stride, const uint32_t* __restrict__ labels,
    const int32_t* __restrict__ island, int64_t Ns, const CapShape* __restrict__ shapes, int S, int spb, int n_domains,
    unsigned long long* __restrict__ dom_slots, uint32_t* __restrict__ dom_nodes) {
  __shared__ unsigned long long s_acc[DM_ACC];
  __shared__ uint32_t s_key[DM_HASH];
  __shared__ uint16_t s_lid[DM_HASH];
  __shared__ uint32_t s_dom[CP_SPAN];
  __shared__ uint32_t s_nd;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < DM_HASH; i += CP_THREADS) s_key[i] = DM_EMPTY;
  for (int i = tid; i < DM_ACC; i += CP_THREADS) s_acc[i] = 0;
  if (tid == 0) s_nd = 0;
  // the block's nodes: a lane past the shard holds what the SoA's padding holds (NEVER, no labels, no domain)
  int64_t r[CP_NPT][D];
  uint32_t lab[CP_NPT];
  int dom[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) {
    const int64_t n = (int64_t)blockIdx.x * CP_SPAN + tid * CP_NPT + k;
    const bool in = n < Ns;
#pragma unroll
    for (int d = 0; d < D; ++d) r[k][d] = in ? res[(int64_t)d * stride + n] : NEVER;
    lab[k] = in ? labels[n] : 0u;
    const int id = in ? island[n] : -1;
    dom[k] = (id >= 0 && id < n_domains) ? id : -1;
  }
  __syncthreads();
  // 1. dictionary: hs[k] = the key's place in the table
  int hs[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) {
    hs[k] = -1;
    if (dom[k] < 0) continue;
    if (k > 0 && dom[k] == dom[k - 1]) {
      hs[k] = hs[k - 1];
      continue;
    }
    const uint32_t id = (uint32_t)dom[k];
    uint32_t h = (id * 2654435761u) >> (32 - DM_HASH_BITS);
    for (;;) {   // ends: the table has twice the slots the block has nodes
      const uint32_t prev = atomicCAS(&s_key[h], DM_EMPTY, id);
      if (prev == DM_EMPTY) {
        const uint32_t l = atomicAdd(&s_nd, 1u);   // < CP_SPAN: one per distinct id of the block
        s_lid[h] = (uint16_t)l;
        s_dom[l] = id;
        break;
      }
      if (prev == id) break;
      h = (h + 1) & (DM_HASH - 1);
    }
    hs[k] = (int)h;
  }
  __syncthreads();
  const int nd = (int)s_nd;
  if (nd == 0) return;   // block-uniform: no node of this block has a domain
  int slot[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) slot[k] = hs[k] >= 0 ? (int)s_lid[hs[k]] : -1;
  // 2. reduction widths (wave-uniform)
  bool same = true;
#pragma unroll
  for (int k = 1; k < CP_NPT; ++k) same &= slot[k] == slot[0];
  const bool kfold = __builtin_amdgcn_ballot_w64(!same) == 0;
  int w[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) w[k] = __builtin_amdgcn_readfirstlane(uniform_width(slot[k]));
  const int tb = min(CP_TS, DM_ACC / nd);   // nd <= CP_SPAN <= DM_ACC: at least one shape
  const int s_begin = blockIdx.y * spb;
  const int s_end = min(S, s_begin + spb);
  for (int t0 = s_begin; t0 < s_end; t0 += tb) {
    const int nt = min(tb, s_end - t0);
    for (int t = 0; t < nt; ++t) {
      const CapShape sp = shapes[t0 + t];   // wave-uniform: scalar loads, the record lives in SGPRs
      bool fit[CP_NPT];
      uint64_t c[CP_NPT];
      cap_eval<CP_NPT>(sp, r, lab, fit, c);
      if (SLICE && sp.pad_[0] != 0) {   // uniform: a node-level row
#pragma unroll
        for (int k = 0; k < CP_NPT; ++k) {
          c[k] = slice_units((uint32_t)c[k], sp.pad_[0]);   // cap <= CP_CAP_MAX: a 32-bit division
          fit[k] &= c[k] >= 1;
        }
      }
      unsigned long long* acc = s_acc + t * nd;   // (t + 1) * nd <= tb * nd <= DM_ACC
      uint64_t v[CP_NPT];
#pragma unroll
      for (int k = 0; k < CP_NPT; ++k) v[k] = fit[k] ? ((uint64_t(1) << DM_CNT_SHIFT) | c[k]) : 0;
      if (kfold) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < CP_NPT; ++k) x += v[k];
        x = group_sum_u64(x, w[0]);
        if (slot[0] >= 0 && (lane & (w[0] - 1)) == 0 && x != 0) atomicAdd(&acc[slot[0]], (unsigned long long)x);
      } else {
#pragma unroll
        for (int k = 0; k < CP_NPT; ++k) {
          const uint64_t x = group_sum_u64(v[k], w[k]);
          if (slot[k] >= 0 && (lane & (w[k] - 1)) == 0 && x != 0) atomicAdd(&acc[slot[k]], (unsigned long long)x);
        }
      }
    }
    __syncthreads();
    // 4. flush the nt * nd accumulators
    const uint32_t tot = (uint32_t)(nt * nd);
    for (uint32_t i = (uint32_t)tid; i < tot; i += CP_THREADS) {
      const uint64_t x = s_acc[i];
      if (x == 0) continue;
      s_acc[i] = 0;
      const uint32_t t = i / (uint32_t)nd, l = i - t * (uint32_t)nd;
      const int64_t at = (int64_t)(t0 + (int)t) * n_domains + s_dom[l];   // row < S, column < n_domains
      atomicAdd(&dom_slots[at], (unsigned long long)(x & DM_SUM_MASK));
      if (dom_nodes) atomicAdd(&dom_nodes[at], (uint32_t)(x >> DM_CNT_SHIFT));   // uniform: NULL = not asked for
    }
    __syncthreads();
  }
}

}  // namespace

}  // namespace pe
