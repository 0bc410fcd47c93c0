// The Appendix-B key on the device, shared by the greedy's scan / walk kernels (pe_kernels.hip) and the
// domain placement kernel (pe_place.hip): one statement of the rule for every kernel that scores a node.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pe_kernels.h"

namespace pe {

// Appendix B key: fit ? (score << 24) | gid : NO_KEY, score = min(a+b+c+d, 2^40-1) with
// a = left_cpu, b = left_mem >> 20, c = left_gpu << 20, d = left_eph >> 24, each term saturated.
__device__ __forceinline__ uint64_t node_key(int64_t r0, int64_t r1, int64_t r2, int64_t r3, uint32_t lab,
                                             int64_t q0, int64_t q1, int64_t q2, int64_t q3, uint32_t need,
                                             uint64_t gid) {
  const bool fit = ((lab & need) == need) & (q0 <= r0) & (q1 <= r1) & (q2 <= r2) & (q3 <= r3);
  const uint64_t a = (uint64_t)r0 - (uint64_t)q0;
  const uint64_t b = ((uint64_t)r1 - (uint64_t)q1) >> 20;
  const uint64_t c = (uint64_t)r2 - (uint64_t)q2;
  const uint64_t d = ((uint64_t)r3 - (uint64_t)q3) >> 24;
  const bool big = (a > SCORE_MAX) | (b > SCORE_MAX) | (c >= (1ull << 20)) | (d > SCORE_MAX);
  const uint64_t sum = a + b + (c << 20) + d;      // < 2^42 whenever !big
  const uint64_t score = (big | (sum > SCORE_MAX)) ? SCORE_MAX : sum;
  return fit ? ((score << 24) | gid) : NO_KEY;
}

}  // namespace pe
