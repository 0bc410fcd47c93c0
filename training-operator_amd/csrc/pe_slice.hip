// pe_gang_slice_tree on the device (include/placement.h): a gang of slices of z pods, each slice inside one
// domain of level sl or inside one node.  The tables hold one row per distinct (shape, z, sl) (pe_slice_plan.h):
// SLOTS below the level m = max(sl, 0), UNITS -- whole slices -- at and above it.  The roll-up in between is
// pe_tree.hip's tree_rollup_kernel as it is: the units of a level above m are the sum of the children's units.
//
// slice_leaf_kernel: gang_capacity_domains_kernel's body (pe_domains_body.h) with the one difference that a
//   node-level row adds floor(cap / z) of every node, and only of nodes that hold a slice.  The other rows
//   leave it in slots.  No node table.
// slice_units_kernel: the conversion at level sl >= 0, in place: block (x, y) takes columns [256 y, 256 y + 256)
//   of row x of one level and divides them by the row's z when the row's sl is that level (block-uniform: the
//   others return).
//   Launched for level 0 after the leaf kernel and for level l after its roll-up, and only for levels some row
//   of the call names.
// slice_select_kernel: tree_select_kernel's scan, from the pick's level m upward and without the per-level
//   counts; one wave per pick, four per block.
// slice_split_kernel: tree_split_kernel's descent (pe_split_level.h) with the pick's list multiplied by z when
//   it arrives at level m: the steps above m hand out units, the steps below it pods.  a * z <= slots(m, D)
//   because a <= floor(slots / z), so every step keeps its premise.  3 * max_parts * 8 B of dynamic LDS.
// Integers only, every choice by (value, id), none by lane; the only atomics are the leaf flush's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pe_domains_body.h"
#include "pe_kernels.h"
#include "pe_slice_plan.h"
#include "pe_split_level.h"
#include "pe_split_plan.h"

namespace pe {

namespace {

__global__ __launch_bounds__(CP_THREADS) void slice_leaf_kernel(
    const int64_t* __restrict__ res, int64_t stride, const uint32_t* __restrict__ labels,
    const int32_t* __restrict__ island, int64_t Ns, const CapShape* __restrict__ shapes, int S, int spb, int n_domains,
    unsigned long long* __restrict__ dom_units) {
  gang_capacity_domains_body<true>(res, stride, labels, island, Ns, shapes, S, spb, n_domains, dom_units, nullptr);
}

constexpr int SU_THREADS = 256;

__global__ __launch_bounds__(SU_THREADS) void slice_units_kernel(unsigned long long* __restrict__ table, int64_t pitch,
                                                                 int n_cols, const SliceRow* __restrict__ rows,
                                                                 int level) {
  const SliceRow row = rows[blockIdx.x];   // block-uniform
  if (row.sl != level || row.z == 1) return;
  const int k = (int)(blockIdx.y * SU_THREADS + threadIdx.x);
  if (k >= n_cols) return;
  unsigned long long* const cell = table + (int64_t)blockIdx.x * pitch + k;   // row < the launch's rows, k < n_cols
  *cell = slice_units(*cell, (uint32_t)row.z);
}

__global__ __launch_bounds__(256) void slice_select_kernel(const unsigned long long* __restrict__ leaf_units,
                                                           const unsigned long long* __restrict__ upper_units, int r0,
                                                           int R, TreeLevels lv, const TreePick* __restrict__ picks,
                                                           int P, TreeSel* __restrict__ out) {
  const int p = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  const TreePick pk = picks[p];   // shape: the row; count: the units wanted; pad_: the lowest level m
  const int64_t s = (int64_t)pk.shape - r0;
  if (s < 0 || s >= R) return;   // a row of another launch
  const uint64_t want = (uint64_t)pk.count;   // >= 1
  uint64_t a_units = 0;
  int32_t a_dom = -1, a_level = -1;
#pragma unroll
  for (int l = 0; l < TR_MAX_LEVELS; ++l) {
    if (l < pk.pad_ || l > pk.max_level || a_level >= 0) continue;   // wave-uniform
    const int n = lv.size[l];
    const unsigned long long* row = l == 0 ? leaf_units + s * n : upper_units + s * lv.pitch + lv.col[l];
    uint64_t best = ~uint64_t(0);
    uint32_t bk = ~0u;
    for (int k = lane; k < n; k += 64) {
      const uint64_t x = row[k];
      if (x >= want && x < best) {   // k ascends: the first of equal values stays
        best = x;
        bk = (uint32_t)k;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t ob = __shfl_xor(best, o, 64);
      const uint32_t ok = __shfl_xor(bk, o, 64);
      if (ob < best || (ob == best && ok < bk)) {
        best = ob;
        bk = ok;
      }
    }
    if (bk != ~0u) {   // the lowest level that holds the slices
      a_units = best;
      a_dom = (int32_t)bk;
      a_level = l;
    }
  }
  if (lane == 0) out[p] = TreeSel{a_units, a_dom, a_level};   // none: 0, -1, -1
}

__global__ __launch_bounds__(64) void slice_split_kernel(const unsigned long long* __restrict__ leaf_units,
                                                         const unsigned long long* __restrict__ upper_units, int r0,
                                                         int R, TreeLevels lv, SplitCsr csr,
                                                         const int32_t* __restrict__ plan,
                                                         const SliceRow* __restrict__ rows,
                                                         const TreePick* __restrict__ picks,
                                                         const TreeSel* __restrict__ sel, int p0, int n, int max_parts,
                                                         int32_t* __restrict__ buf) {
  extern __shared__ int2 slice_lds[];
  const int k = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (k >= n) return;
  const TreePick pk = picks[p0 + k];
  const int64_t s = (int64_t)pk.shape - r0;
  if (s < 0 || s >= R) return;   // a row of another launch
  const TreeSel a = sel[p0 + k];
  const int z = rows[pk.shape].z, m = pk.pad_;
  int2* src = slice_lds;
  int2* dst = slice_lds + max_parts;
  int2* const tmp = slice_lds + 2 * max_parts;
  int np = 0;
  int32_t spread[TR_MAX_LEVELS] = {0, 0, 0, 0};
  if (a.level >= 0) {
    if (lane == 0) src[0] = make_int2(a.domain, pk.count);
    np = 1;
    __syncthreads();
#pragma unroll
    for (int l = TR_MAX_LEVELS - 1; l >= 0; --l) {
      if (l > a.level || np < 0) continue;
      spread[l] = np;
      if (l == m && z != 1) {   // S_m from units to pods: a * z <= count < 2^31
        for (int i = lane; i < np; i += 64) src[i].y *= z;
        __syncthreads();
      }
      if (l == 0) continue;
      const unsigned long long* row =
          l == 1 ? leaf_units + s * lv.size[0] : upper_units + s * lv.pitch + lv.col[l - 1];
      np = split_level(row, plan + csr.start_at[l], plan + csr.child_at[l], src, dst, tmp, np, max_parts, lane);
      int2* const sw = src;
      src = dst;
      dst = sw;
    }
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

hipError_t launch_slice_leaf(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                             const int32_t* island, int64_t Ns, const CapShape* shapes, int64_t R, int n_domains,
                             uint64_t* dom_units) {
  if (R <= 0 || Ns <= 0) return hipSuccess;
  const int64_t gx = cap_node_blocks(Ns);
  // as launch_gang_capacity_domains: split the rows when the shard alone has too few node blocks
  int64_t gy = std::min<int64_t>(R, std::max<int64_t>(1, 2048 / gx));
  const int64_t spb = (R + gy - 1) / gy;
  gy = (R + spb - 1) / spb;
  hipLaunchKernelGGL(slice_leaf_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(CP_THREADS), 0, s, res, stride, labels,
                     island, Ns, shapes, (int)R, (int)spb, n_domains, (unsigned long long*)dom_units);
  return hipGetLastError();
}

hipError_t launch_slice_units(hipStream_t s, uint64_t* table, int64_t pitch, int n_cols, const SliceRow* rows, int64_t R,
                              int level) {
  if (R <= 0 || n_cols <= 0) return hipSuccess;
  if (R > (int64_t)INT32_MAX || n_cols > DM_MAX_DOMAINS) return hipErrorInvalidValue;   // grid.y: 256 at most
  hipLaunchKernelGGL(slice_units_kernel, dim3((unsigned)R, (unsigned)((n_cols + SU_THREADS - 1) / SU_THREADS)),
                     dim3(SU_THREADS), 0, s, (unsigned long long*)table, pitch, n_cols, rows, level);
  return hipGetLastError();
}

hipError_t launch_slice_select(hipStream_t s, const uint64_t* leaf_units, const uint64_t* upper_units, int64_t r0,
                               int64_t R, const TreeLevels& levels, const TreePick* picks, int64_t P, TreeSel* out) {
  if (P <= 0 || R <= 0) return hipSuccess;
  hipLaunchKernelGGL(slice_select_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s,
                     (const unsigned long long*)leaf_units, (const unsigned long long*)upper_units, (int)r0, (int)R, levels,
                     picks, (int)P, out);
  return hipGetLastError();
}

hipError_t launch_slice_split(hipStream_t s, const uint64_t* leaf_units, const uint64_t* upper_units, int64_t r0,
                              int64_t R, const TreeLevels& levels, const SplitCsr& csr, const int32_t* plan,
                              const SliceRow* rows, const TreePick* picks, const TreeSel* sel, int64_t p0, int64_t n,
                              int max_parts, int32_t* buf) {
  if (n <= 0 || R <= 0) return hipSuccess;
  if (max_parts < 1 || max_parts > SPLIT_MAX_PARTS || n > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  const size_t lds = (size_t)3 * (size_t)max_parts * sizeof(int2);
  hipLaunchKernelGGL(slice_split_kernel, dim3((unsigned)n), dim3(64), lds, s, (const unsigned long long*)leaf_units,
                     (const unsigned long long*)upper_units, (int)r0, (int)R, levels, csr, plan, rows, picks, sel,
                     (int)p0, (int)n, max_parts, buf);
  return hipGetLastError();
}

}  // namespace pe
