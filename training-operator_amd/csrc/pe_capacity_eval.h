// The per-node capacity evaluation of pe_domains.hip: gang_capacity_kernel's (pe_capacity.hip), statement
// for statement.  That kernel keeps its own copy: calling this one from it changed its register
// allocation (98 -> 100 VGPRs), and its ISA is what section 14 of DESIGN.md measured.  For one shape
// record, held in SGPRs, and the NPT nodes a thread keeps in registers
//   fit[k] = fit(shape, node k)     c[k] = min(CP_CAP_MAX, min over d with q_d > 0 of floor(res_d / q_d))
// c[k] means something only where fit[k]: a node that does not fit may hold a negative residual, whose
// quotient is never used.  Reciprocal multiply (pe_divmagic.h), no division.
#pragma once
#include <hip/hip_runtime.h>

#include "pe_divmagic.h"
#include "pe_kernels.h"

namespace pe {

template <int NPT>
__device__ __forceinline__ void cap_eval(const CapShape& sp, const int64_t (&r)[NPT][D], const uint32_t (&lab)[NPT],
                                         bool (&fit)[NPT], uint64_t (&c)[NPT]) {
  const uint32_t need = sp.need;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    fit[k] = (lab[k] & need) == need;
    c[k] = CP_CAP_MAX;
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int64_t q = sp.q[d];
#pragma unroll
    for (int k = 0; k < NPT; ++k) fit[k] &= q <= r[k][d];
    if (q > 0) {   // uniform; a zero request bounds nothing (the fit test covers res_d >= 0)
      const uint64_t m = sp.m[d];
      const uint32_t sh = sp.sh[d];
      if (sh >= 64) {   // uniform: every request but 1
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          const uint64_t x = div_by_magic_hi((uint64_t)r[k][d], m, sh);
          c[k] = x < c[k] ? x : c[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
          const uint64_t x = div_by_magic((uint64_t)r[k][d], m, sh);
          c[k] = x < c[k] ? x : c[k];
        }
      }
    }
  }
}

}  // namespace pe
