// libplacement: the device half of pe_release_gangs / pe_assume_gangs.  The host walks every pod slot for its mirror
// anyway (pe_ledger_plan.h), so the exact residuals of every touched node are known before the launch: the kernel
// only scatters them into res[4][stride].  One thread per record in a grid-stride loop, five 8-B loads and four 8-B
// stores; the locals of a launch are distinct, nothing is read back and nothing is added, so the launch is
// idempotent and needs no atomic.  Ordinary vector stores and plain C++ only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pe_kernels.h"

namespace pe {

__global__ __launch_bounds__(LG_THREADS) void ledger_scatter_kernel(int64_t* __restrict__ res, int64_t stride,
                                                                    const LedgerRec* __restrict__ recs, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * LG_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * LG_THREADS + threadIdx.x; i < n; i += step) {
    const LedgerRec r = recs[i];
#pragma unroll
    for (int d = 0; d < D; ++d) res[d * stride + r.local] = r.res[d];
  }
}

hipError_t launch_ledger_scatter(hipStream_t s, int64_t* res, int64_t stride, const LedgerRec* recs, int64_t n) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n + LG_THREADS - 1) / LG_THREADS, LG_MAX_BLOCKS);
  hipLaunchKernelGGL(ledger_scatter_kernel, dim3((unsigned)blocks), dim3(LG_THREADS), 0, s, res, stride, recs, n);
  return hipGetLastError();
}

}  // namespace pe
