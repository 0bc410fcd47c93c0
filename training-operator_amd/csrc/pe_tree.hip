// Gang capacity over a topology hierarchy (pe_gang_capacity_tree, and pe_gang_capacity_domains as its
// one-level case): the leaf table of pe_domains.hip ([shape][leaf domain] slots and nodes) rolled up along
// the caller's parent map, level by level, and the selection that walks the levels.  The plan
// (pe_tree_plan.h) gives per upper level a CSR of child lists and the lanes per parent.
//
// tree_rollup_kernel: one launch per upper level.  A group of w lanes (w a power of two <= 64, so a group
// never leaves its wave) owns one (shape, parent): its lanes stride over the parent's child list, gather
// the children's slots (u64) and nodes (u32) from the shape's lower row, a log2(w)-step butterfly folds the
// group and lane 0 of the group stores both values.  Every (shape, parent) is stored, a childless parent as
// 0: the upper table needs no zeroing, and there are no atomics.  Integers throughout: no result depends on
// an order.
// tree_select_kernel: one wave per distinct (shape, count, max_level).  Per level the wave scans the
// shape's row for the lexicographic minimum of (slots, id) among the values >= count and counts them; the
// answer is that of the first level <= max_level that has one, the counts of all levels are stored.
#include <hip/hip_runtime.h>

#include "pe_kernels.h"
#include "pe_wave.h"

namespace pe {

namespace {

constexpr int TR_THREADS = 256;

__global__ __launch_bounds__(TR_THREADS) void tree_rollup_kernel(
    const unsigned long long* __restrict__ lo_slots, const uint32_t* __restrict__ lo_nodes, int64_t lo_pitch,
    const int32_t* __restrict__ start, const int32_t* __restrict__ child, uint32_t n_parents, int w, int wshift,
    uint32_t groups, unsigned long long* __restrict__ up_slots, uint32_t* __restrict__ up_nodes, int64_t up_pitch) {
  const uint32_t t = blockIdx.x * (uint32_t)TR_THREADS + threadIdx.x;   // groups * w <= 2^31 (the launcher checks)
  const uint32_t g = t >> wshift;
  const int sub = (int)(t & (uint32_t)(w - 1));
  const bool live = g < groups;   // a dead group still takes part in the butterfly
  const uint32_t s = live ? g / n_parents : 0u;
  const uint32_t p = live ? g - s * n_parents : 0u;
  uint64_t sum = 0;
  uint32_t cnt = 0;
  if (live) {
    const int e = start[p + 1];
    const unsigned long long* srow = lo_slots + (int64_t)s * lo_pitch;
    if (lo_nodes) {   // uniform: NULL = the node table was not asked for
      const uint32_t* nrow = lo_nodes + (int64_t)s * lo_pitch;
      for (int i = start[p] + sub; i < e; i += w) {
        const int c = child[i];   // < the lower level's size: the plan validated the map
        sum += srow[c];
        cnt += nrow[c];
      }
    } else {
      for (int i = start[p] + sub; i < e; i += w) sum += srow[child[i]];
    }
  }
  sum = group_sum_u64(sum, w);
  if (lo_nodes) cnt = group_sum_u32(cnt, w);
  if (live && sub == 0) {
    const int64_t at = (int64_t)s * up_pitch + p;   // s < S, p < n_parents
    up_slots[at] = sum;
    if (up_nodes) up_nodes[at] = cnt;
  }
}

__global__ __launch_bounds__(256) void tree_select_kernel(const unsigned long long* __restrict__ leaf_slots,
                                                          const unsigned long long* __restrict__ upper_slots, int s0,
                                                          int S, TreeLevels lv, const TreePick* __restrict__ picks,
                                                          int P, TreeSel* __restrict__ out,
                                                          uint32_t* __restrict__ feasible) {
  const int p = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const TreePick pk = picks[p];
  const int64_t s = (int64_t)pk.shape - s0;
  if (s < 0 || s >= S) return;   // a row of another launch
  const uint64_t count = (uint64_t)pk.count;   // >= 1
  uint64_t a_slots = 0;
  int32_t a_dom = -1, a_level = -1;
#pragma unroll
  for (int l = 0; l < TR_MAX_LEVELS; ++l) {
    if (l >= lv.n_levels) break;
    const int n = lv.size[l];
    const unsigned long long* row = l == 0 ? leaf_slots + s * n : upper_slots + s * lv.pitch + lv.col[l];
    uint64_t best = ~uint64_t(0);
    uint32_t bk = ~0u, feas = 0;
    for (int k = lane; k < n; k += 64) {
      const uint64_t x = row[k];
      if (x >= count) {
        ++feas;
        if (x < best) {   // k ascends: the first of equal values stays
          best = x;
          bk = (uint32_t)k;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t ob = __shfl_xor(best, o, 64);
      const uint32_t ok = __shfl_xor(bk, o, 64);
      feas += __shfl_xor(feas, o, 64);
      if (ob < best || (ob == best && ok < bk)) {
        best = ob;
        bk = ok;
      }
    }
    if (lane == 0) feasible[(int64_t)p * lv.n_levels + l] = feas;
    if (a_level < 0 && l <= pk.max_level && feas > 0) {   // the lowest level that holds the gang
      a_slots = best;
      a_dom = (int32_t)bk;
      a_level = l;
    }
  }
  if (lane == 0) out[p] = TreeSel{a_slots, a_dom, a_level};   // none: 0, -1, -1
}

}  // namespace

hipError_t launch_tree_rollup(hipStream_t s, const uint64_t* lo_slots, const uint32_t* lo_nodes, int64_t lo_pitch,
                              const int32_t* start, const int32_t* child, int n_parents, int width, int64_t S,
                              uint64_t* up_slots, uint32_t* up_nodes, int64_t up_pitch) {
  if (S <= 0 || n_parents <= 0) return hipSuccess;
  int wshift = 0;
  while ((1 << wshift) < width) ++wshift;
  const int64_t groups = S * n_parents;
  const int64_t threads = groups << wshift;
  if (width < 1 || width > 64 || (1 << wshift) != width || threads > (int64_t(1) << 31)) return hipErrorInvalidValue;
  const int64_t blocks = (threads + TR_THREADS - 1) / TR_THREADS;
  hipLaunchKernelGGL(tree_rollup_kernel, dim3((unsigned)blocks), dim3(TR_THREADS), 0, s,
                     (const unsigned long long*)lo_slots, lo_nodes, lo_pitch, start, child, (uint32_t)n_parents, width,
                     wshift, (uint32_t)groups, (unsigned long long*)up_slots, up_nodes, up_pitch);
  return hipGetLastError();
}

hipError_t launch_tree_select(hipStream_t s, const uint64_t* leaf_slots, const uint64_t* upper_slots, int64_t s0,
                              int64_t S, const TreeLevels& levels, const TreePick* picks, int64_t P, TreeSel* out,
                              uint32_t* feasible) {
  if (P <= 0 || S <= 0) return hipSuccess;
  hipLaunchKernelGGL(tree_select_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s,
                     (const unsigned long long*)leaf_slots, (const unsigned long long*)upper_slots, (int)s0, (int)S, levels,
                     picks, (int)P, out, feasible);
  return hipGetLastError();
}

}  // namespace pe
