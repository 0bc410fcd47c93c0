// pe_gang_split_tree's descent (include/placement.h): the gang of a pick, selected into one domain of one
// level by tree_select_kernel (pe_tree.hip), spread over the fewest domains of every level below, down to
// (leaf, pods) parts.  Runs after the selection on the same device tables, picks and answers.
//
// tree_split_kernel: one wave (a block of 64 threads) per pick.  The lists S_l and S_{l-1} of (domain, pods)
// ping-pong in LDS, a third list takes a parent's whole parts before they are ordered: 3 * max_parts * 8 B of
// dynamic LDS, 24 KiB at PE_MAX_SPLIT_PARTS.  Per (parent, allotment a) of S_l the lanes stride over the
// parent's child list (the plan's CSR, ascending ids) in the threshold form of the rule (pe_split_plan.h); the
// step itself, split_level, lives in pe_split_level.h, which pe_slice.hip shares:
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
#include "pe_split_level.h"
#include "pe_split_plan.h"

namespace pe {

namespace {

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
