// Why a shape fits no node (pe_fit_explain): per distinct (request, need, domain) record the shard's live nodes
// in the record's scope, counted by 5-bit signature
//   bit d (0 .. 3) = req_d > res_d(n) (signed int64)      bit 4 = (labels(n) & need) != need
// and per dimension d the nearest miss: the minimum of req_d - res_d(n), as an exact u64, over the nodes whose
// signature is exactly 1 << d.  Read-only and integers throughout: no result depends on any order.
//
// fit_explain_kernel: block (x, y) owns CP_SPAN nodes (CP_NPT per thread, loaded once, coalesced from the SoA,
// kept in registers with their labels and level-domain) and the records [y * spb, (y + 1) * spb); a record is
// read through a wave-uniform address and lives in SGPRs.  Per record and node slot five compares give five
// wave ballots (uniform 64-bit masks), and LANE b (mod 32) counts BIN b: it ANDs the scope mask with each
// ballot or its complement, as bit d of b says, and takes the popcount -- 32 bins in 64 lanes at once on the
// vector unit (4 x 2 halves of xor + and per slot), nothing per node touches LDS.  The 62-mask binary tree on the
// scalar unit costs 94 scalar instructions per 64 nodes, and a CU's four SIMDs share ONE scalar unit: that
// form is bound by it at four waves per block, this one spreads over the four vector units.
// Near values: a lane folds its own nodes; a dimension is reduced over the wave only when some node of the wave
// has the exclusive signature (a uniform branch on the ballot), and the whole part is compiled out when the
// caller wants no near values.  A wave parks its 32 counts and 4 minima in LDS; after every EX_TS records the
// block folds its waves and adds what is non-zero to the [S][32] / [S][4] tables with integer global atomics
// (atomicAdd u64, atomicMin u64).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pe_explain_plan.h"
#include "pe_kernels.h"

namespace pe {

static_assert(EX_DIMS == D, "the signature has one bit per resource dimension");

namespace {

constexpr int EX_WAVES = CP_THREADS / 64;
constexpr uint64_t EX_NONE = ~uint64_t(0);   // no node with the exclusive signature (a true value is <= 2^64 - 2)

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

template <bool NEAR, bool DOM>
__global__ __launch_bounds__(CP_THREADS) void fit_explain_kernel(const int64_t* __restrict__ res, int64_t stride,
                                                                 const uint32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ island, int64_t Ns,
                                                                 const int32_t* __restrict__ leaf_dom, int n_leaf,
                                                                 const ExplainRec* __restrict__ recs, int S, int spb,
                                                                 uint64_t* __restrict__ hist,
                                                                 uint64_t* __restrict__ near) {
  __shared__ uint32_t s_cnt[EX_TS][EX_WAVES][EX_BINS];
  __shared__ uint64_t s_near[NEAR ? EX_TS : 1][EX_WAVES][D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the block's nodes: a lane past the shard holds what the SoA's padding holds (NEVER, no labels, no domain);
  // a removed slot holds NEVER in dimension 0 as well.  Neither is live.
  int64_t r[CP_NPT][D];
  uint32_t lab[CP_NPT];
  int32_t dm[CP_NPT];
  bool live[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) {
    const int64_t n = (int64_t)blockIdx.x * CP_SPAN + k * CP_THREADS + threadIdx.x;
    const bool in = n < Ns;
#pragma unroll
    for (int d = 0; d < D; ++d) r[k][d] = in ? res[(int64_t)d * stride + n] : NEVER;
    lab[k] = in ? labels[n] : 0u;
    live[k] = r[k][0] != NEVER;
    dm[k] = EX_NO_DOMAIN;
    if (DOM && in) {
      const int32_t isl = island[n];
      if (isl >= 0 && isl < n_leaf) dm[k] = leaf_dom[isl];
    }
  }
  // lane b (mod 32) counts bin b: per signature bit, all ones where the bin wants the ballot's complement
  uint64_t inv[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) inv[d] = ((lane >> d) & 1) ? uint64_t(0) : ~uint64_t(0);

  const int s_begin = blockIdx.y * spb;
  const int s_end = min(S, s_begin + spb);
  for (int t0 = s_begin; t0 < s_end; t0 += EX_TS) {
    const int nt = min(EX_TS, s_end - t0);
    for (int t = 0; t < nt; ++t) {
      const ExplainRec rec = recs[t0 + t];   // wave-uniform: scalar loads, the record lives in SGPRs
      const uint32_t need = rec.need;
      const int32_t dom = rec.dom;
      uint32_t cnt = 0;
      uint64_t nv[D];
      uint64_t any[D];   // uniform: the wave's nodes with the exclusive signature of d
#pragma unroll
      for (int d = 0; d < D; ++d) {
        nv[d] = EX_NONE;
        any[d] = 0;
      }
#pragma unroll
      for (int k = 0; k < CP_NPT; ++k) {
        const bool scope = live[k] && (!DOM || dom < 0 || dm[k] == dom);
        bool x[5];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = rec.q[d] > r[k][d];
        x[4] = (lab[k] & need) != need;
        uint64_t m = __builtin_amdgcn_ballot_w64(scope);
        uint64_t b[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
          b[d] = __builtin_amdgcn_ballot_w64(x[d]);
          m &= b[d] ^ inv[d];
        }
        cnt += (uint32_t)__popcll(m);
        if (NEAR) {
          const uint64_t sc = __builtin_amdgcn_ballot_w64(scope);
#pragma unroll
          for (int d = 0; d < D; ++d) {
            uint64_t e = sc;
#pragma unroll
            for (int o = 0; o < 5; ++o) e &= o == d ? b[o] : ~b[o];
            any[d] |= e;
            const bool mine = scope && x[d] && !x[(d + 1) & 3] && !x[(d + 2) & 3] && !x[(d + 3) & 3] && !x[4];
            // req_d > res_d here, so the difference of the two's-complement bits is the exact shortfall
            const uint64_t gap = (uint64_t)rec.q[d] - (uint64_t)r[k][d];
            nv[d] = mine && gap < nv[d] ? gap : nv[d];
          }
        }
      }
      if (lane < EX_BINS) s_cnt[t][wave][lane] = cnt;
      if (NEAR) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          uint64_t v = EX_NONE;
          if (any[d] != 0) v = wave_min_u64(nv[d]);   // uniform branch
          if (lane == 0) s_near[t][wave][d] = v;
        }
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nt * EX_BINS; c += CP_THREADS) {
      const int t = c / EX_BINS, bin = c % EX_BINS;
      uint32_t a = 0;
#pragma unroll
      for (int w = 0; w < EX_WAVES; ++w) a += s_cnt[t][w][bin];
      if (a) atomicAdd((unsigned long long*)&hist[(int64_t)(t0 + t) * EX_BINS + bin], (unsigned long long)a);
    }
    if (NEAR) {
      for (int c = threadIdx.x; c < nt * D; c += CP_THREADS) {
        const int t = c / D, d = c % D;
        uint64_t a = EX_NONE;
#pragma unroll
        for (int w = 0; w < EX_WAVES; ++w) a = s_near[t][w][d] < a ? s_near[t][w][d] : a;
        if (a != EX_NONE) atomicMin((unsigned long long*)&near[(int64_t)(t0 + t) * D + d], (unsigned long long)a);
      }
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_fit_explain(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                              const int32_t* island, int64_t Ns, const int32_t* leaf_dom, int n_leaf, bool with_domains,
                              const ExplainRec* recs, int64_t S, uint64_t* hist, uint64_t* near) {
  if (S <= 0 || Ns <= 0) return hipSuccess;
  const int64_t gx = cap_node_blocks(Ns);
  // enough blocks to fill the chip when the shard alone has too few node blocks: split the records
  const int64_t tiles = (S + EX_TS - 1) / EX_TS;
  int64_t gy = std::min<int64_t>(tiles, std::max<int64_t>(1, 2048 / gx));
  const int64_t spb = ((S + gy - 1) / gy + EX_TS - 1) / EX_TS * EX_TS;
  gy = (S + spb - 1) / spb;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(CP_THREADS);
#define PE_EXPLAIN_LAUNCH(NEAR, DOM)                                                                              \
  hipLaunchKernelGGL((fit_explain_kernel<NEAR, DOM>), grid, block, 0, s, res, stride, labels, island, Ns, leaf_dom, \
                     n_leaf, recs, (int)S, (int)spb, hist, near)
  if (near) {
    if (with_domains) PE_EXPLAIN_LAUNCH(true, true);
    else PE_EXPLAIN_LAUNCH(true, false);
  } else {
    if (with_domains) PE_EXPLAIN_LAUNCH(false, true);
    else PE_EXPLAIN_LAUNCH(false, false);
  }
#undef PE_EXPLAIN_LAUNCH
  return hipGetLastError();
}

}  // namespace pe
