// Exact floor(n / d) for 0 <= n < 2^63 by one multiplication with a per-divisor reciprocal (the gang
// capacity kernel divides every residual of a shard by a request that is the same for the whole wave).
//
// For a divisor 1 <= d < 2^63 let l = bit_length(d - 1) (so 2^(l-1) < d <= 2^l, l = 0 for d = 1) and
//   m = floor(2^(63+l) / d) + 1.
// Then 2^(63+l) < m * d <= 2^(63+l) + d, and for every n < 2^63
//   n / d  <=  n * m / 2^(63+l)  <=  n / d + n / 2^(63+l)  <  n / d + 2^-l  <=  n / d + 1 / d,
// so floor(n * m / 2^(63+l)) = floor(n / d): the fraction of n / d is at most (d - 1) / d.
// m < 2^64 because 2^(63+l) / d < 2^64 for d > 2^(l-1) (d = 1: m = 2^63 + 1).  The product n * m is
// below 2^127; its bits from 63 + l upward are the quotient.
//
// Plain C++: the host computes magic() (unsigned __int128), host and device run divide().
#pragma once
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PE_DM_HD __host__ __device__ __forceinline__
#elif defined(__HIPCC__)
#define PE_DM_HD __host__ __device__ inline
#else
#define PE_DM_HD inline
#endif

namespace pe {

struct DivMagic {
  uint64_t m;       // the reciprocal
  uint32_t shift;   // 63 + l, in [63, 126]
};

// d in [1, 2^63).  Host only.
inline DivMagic div_magic(uint64_t d) {
  uint32_t l = 0;
  while (l < 63 && (uint64_t(1) << l) < d) ++l;   // bit_length(d - 1)
  const unsigned __int128 p = (unsigned __int128)1 << (63 + l);
  return DivMagic{(uint64_t)(p / d) + 1, 63 + l};
}

// high 64 bits of a * b
PE_DM_HD uint64_t dm_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(n / d) for n < 2^63 and shift >= 64, i.e. every divisor but 1: the quotient sits in the high
// product word.
PE_DM_HD uint64_t div_by_magic_hi(uint64_t n, uint64_t m, uint32_t shift) { return dm_mulhi(n, m) >> (shift - 64); }

// floor(n / d) for n < 2^63, (m, shift) = div_magic(d).  shift is 63 only for d = 1, where the
// quotient straddles the two product words.
PE_DM_HD uint64_t div_by_magic(uint64_t n, uint64_t m, uint32_t shift) {
  if (shift >= 64) return div_by_magic_hi(n, m, shift);
  return (dm_mulhi(n, m) << 1) | ((n * m) >> 63);
}

}  // namespace pe
