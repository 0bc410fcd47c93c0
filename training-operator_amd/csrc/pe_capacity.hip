// Gang capacity (pe_gang_capacity): per distinct pod shape, how many pods of that shape the shard's
// nodes hold -- sum, largest single node and number of fitting nodes of
//   cap(s, n) = fit(s, n) ? min(CP_CAP_MAX, min over d with q_d > 0 of floor(res_d(n) / q_d)) : 0
// (one pod of shape q lowers floor(res_d / q_d) by one in every such dimension).
//
// The divisor of every division is a request, the same for the whole wave, so the host turns it into a
// 64-bit reciprocal (pe_divmagic.h) and the kernel multiplies: one 64 x 64 -> high-64 product and a
// shift per (shape, node, dimension), no division expansion.
//
// gang_capacity_kernel: block (x, y) owns CP_SPAN nodes (CP_NPT per thread, loaded once, coalesced from
// the SoA, kept in registers) and the shapes [y * spb, (y + 1) * spb); the shape's record is read
// through a wave-uniform address.  Per shape a thread folds its nodes, the wave reduces (sum u64, max
// u32; the node count is a ballot popcount), lane 0 parks the wave's result in LDS, and after every
// CP_TS shapes one thread per shape folds the waves and stores the block's partial.
// gang_capacity_reduce_kernel folds the partials over the node blocks.  Integers throughout: the result
// does not depend on any order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pe_divmagic.h"
#include "pe_kernels.h"

namespace pe {

namespace {

constexpr int CP_WAVES = CP_THREADS / 64;

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(CP_THREADS) void gang_capacity_kernel(const int64_t* __restrict__ res, int64_t stride,
                                                                   const uint32_t* __restrict__ labels, int64_t Ns,
                                                                   const CapShape* __restrict__ shapes, int S, int spb,
                                                                   CapAcc* __restrict__ partials) {
  __shared__ uint64_t s_sum[CP_TS][CP_WAVES];
  __shared__ uint32_t s_max[CP_TS][CP_WAVES];
  __shared__ uint32_t s_cnt[CP_TS][CP_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the block's nodes: a lane past the shard holds what the SoA's padding holds (NEVER, no labels)
  int64_t r[CP_NPT][D];
  uint32_t lab[CP_NPT];
#pragma unroll
  for (int k = 0; k < CP_NPT; ++k) {
    const int64_t n = (int64_t)blockIdx.x * CP_SPAN + k * CP_THREADS + threadIdx.x;
    const bool in = n < Ns;
#pragma unroll
    for (int d = 0; d < D; ++d) r[k][d] = in ? res[(int64_t)d * stride + n] : NEVER;
    lab[k] = in ? labels[n] : 0u;
  }
  const int s_begin = blockIdx.y * spb;
  const int s_end = min(S, s_begin + spb);
  for (int t0 = s_begin; t0 < s_end; t0 += CP_TS) {
    const int nt = min(CP_TS, s_end - t0);
    for (int t = 0; t < nt; ++t) {
      const CapShape sp = shapes[t0 + t];   // wave-uniform: scalar loads, the record lives in SGPRs
      const uint32_t need = sp.need;
      bool fit[CP_NPT];
      uint64_t c[CP_NPT];
#pragma unroll
      for (int k = 0; k < CP_NPT; ++k) {
        fit[k] = (lab[k] & need) == need;
        c[k] = CP_CAP_MAX;
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int64_t q = sp.q[d];
#pragma unroll
        for (int k = 0; k < CP_NPT; ++k) fit[k] &= q <= r[k][d];
        if (q > 0) {   // uniform; a zero request bounds nothing (the fit test covers res_d >= 0)
          const uint64_t m = sp.m[d];
          const uint32_t sh = sp.sh[d];
          // a node that does not fit may hold a negative residual: its quotient is never used
          if (sh >= 64) {   // uniform: every request but 1
#pragma unroll
            for (int k = 0; k < CP_NPT; ++k) {
              const uint64_t x = div_by_magic_hi((uint64_t)r[k][d], m, sh);
              c[k] = x < c[k] ? x : c[k];
            }
          } else {
#pragma unroll
            for (int k = 0; k < CP_NPT; ++k) {
              const uint64_t x = div_by_magic((uint64_t)r[k][d], m, sh);
              c[k] = x < c[k] ? x : c[k];
            }
          }
        }
      }
      uint64_t sum = 0;
      uint32_t mx = 0, cnt = 0;
#pragma unroll
      for (int k = 0; k < CP_NPT; ++k) {
        const uint32_t v = fit[k] ? (uint32_t)c[k] : 0u;
        sum += v;
        mx = v > mx ? v : mx;
        cnt += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(fit[k]));
      }
      sum = wave_sum_u64(sum);
      mx = wave_max_u32(mx);
      if (lane == 0) {
        s_sum[t][wave] = sum;
        s_max[t][wave] = mx;
        s_cnt[t][wave] = cnt;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < nt) {
      CapAcc a{0, 0, 0};
#pragma unroll
      for (int w = 0; w < CP_WAVES; ++w) {
        a.slots += s_sum[threadIdx.x][w];
        a.max_node = max(a.max_node, s_max[threadIdx.x][w]);
        a.nodes += s_cnt[threadIdx.x][w];
      }
      partials[(int64_t)blockIdx.x * S + t0 + threadIdx.x] = a;
    }
    __syncthreads();
  }
}

// out[s] = fold over the gx node blocks of partials[x * S + s]: 16 shapes x 16 block slices per block.
__global__ __launch_bounds__(256) void gang_capacity_reduce_kernel(const CapAcc* __restrict__ partials, int64_t gx,
                                                                   int S, CapAcc* __restrict__ out) {
  __shared__ CapAcc s_acc[16][16];
  const int si = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int s = blockIdx.x * 16 + si;
  CapAcc a{0, 0, 0};
  if (s < S)
    for (int64_t x = sl; x < gx; x += 16) {
      const CapAcc p = partials[x * S + s];
      a.slots += p.slots;
      a.max_node = max(a.max_node, p.max_node);
      a.nodes += p.nodes;
    }
  s_acc[sl][si] = a;
  __syncthreads();
  if (sl == 0 && s < S) {
    for (int w = 1; w < 16; ++w) {
      const CapAcc p = s_acc[w][si];
      a.slots += p.slots;
      a.max_node = max(a.max_node, p.max_node);
      a.nodes += p.nodes;
    }
    out[s] = a;
  }
}

}  // namespace

hipError_t launch_gang_capacity(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                                const CapShape* shapes, int64_t S, CapAcc* partials, CapAcc* out) {
  if (S <= 0 || Ns <= 0) return hipSuccess;
  const int64_t gx = cap_node_blocks(Ns);
  // enough blocks to fill the chip when the shard alone has too few node blocks: split the shapes
  const int64_t tiles = (S + CP_TS - 1) / CP_TS;
  int64_t gy = std::min<int64_t>(tiles, std::max<int64_t>(1, 2048 / gx));
  const int64_t spb = ((S + gy - 1) / gy + CP_TS - 1) / CP_TS * CP_TS;
  gy = (S + spb - 1) / spb;
  hipLaunchKernelGGL(gang_capacity_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(CP_THREADS), 0, s, res, stride,
                     labels, Ns, shapes, (int)S, (int)spb, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gang_capacity_reduce_kernel, dim3((unsigned)((S + 15) / 16)), dim3(256), 0, s, partials, gx,
                     (int)S, out);
  return hipGetLastError();
}

}  // namespace pe
