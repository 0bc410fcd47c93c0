// pe_divmagic.h against unsigned __int128 division: stand-alone (own main), built with the address and
// undefined-behaviour sanitizers by tests/test_divmagic_cpu.py.
//   divisors:   1, 2, 3, 10, 2^k, 2^k +- 1 (k <= 62), 10^18, 2^63 - 2, 2^63 - 1 and seeded random ones of
//               every bit length
//   numerators: 0, 1, d - 1, d, d + 1, 2d - 1, 2d, the largest multiple of d below 2^63 and its
//               predecessor, 2^63 - 1 (those below 2^63), and random ones
// Every divisor's reciprocal must fit 64 bits (m < 2^64 is checked on the 128-bit value).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pe_divmagic.h"

namespace {

using u128 = unsigned __int128;
constexpr uint64_t kTop = (uint64_t(1) << 63) - 1;   // the largest numerator, 2^63 - 1

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

long long failures = 0, checks = 0;

void check(uint64_t n, uint64_t d, const pe::DivMagic& dm) {
  const uint64_t want = (uint64_t)((u128)n / d);
  const uint64_t got = pe::div_by_magic(n, dm.m, dm.shift);
  ++checks;
  if (got != want || (dm.shift >= 64 && pe::div_by_magic_hi(n, dm.m, dm.shift) != want)) {
    if (failures++ < 20)
      std::printf("MISMATCH n=%llu d=%llu: got %llu want %llu (m=%llu shift=%u)\n", (unsigned long long)n,
                  (unsigned long long)d, (unsigned long long)got, (unsigned long long)want, (unsigned long long)dm.m,
                  dm.shift);
  }
}

void check_divisor(uint64_t d) {
  const pe::DivMagic dm = pe::div_magic(d);
  // the definition, in 128 bits: l = bit_length(d - 1), m = floor(2^(63+l) / d) + 1 < 2^64
  unsigned l = 0;
  while (l < 64 && ((u128)1 << l) < d) ++l;
  const u128 m = ((u128)1 << (63 + l)) / d + 1;
  ++checks;
  if ((m >> 64) != 0 || (uint64_t)m != dm.m || dm.shift != 63 + l || dm.shift < 63 || dm.shift > 126) {
    if (failures++ < 20)
      std::printf("BAD MAGIC d=%llu: m=%llu shift=%u (l=%u, m fits 64 bits: %d)\n", (unsigned long long)d,
                  (unsigned long long)dm.m, dm.shift, l, (int)((m >> 64) == 0));
    return;
  }
  const uint64_t top_mult = kTop / d * d;   // the largest multiple of d below 2^63
  const u128 cand[] = {0, 1, (u128)d - 1, d, (u128)d + 1, 2 * (u128)d - 1, 2 * (u128)d, top_mult,
                       top_mult ? top_mult - 1 : 0, kTop, kTop - 1};
  for (u128 n : cand)
    if (n <= kTop) check((uint64_t)n, d, dm);
  for (int i = 0; i < 24; ++i) {
    check(rnd() >> 1, d, dm);                            // anywhere below 2^63
    check(rnd() >> (1 + rnd() % 63), d, dm);             // every magnitude
    const uint64_t k = rnd() % (kTop / d + 1);           // around a random multiple
    const uint64_t base = k * d;
    check(base, d, dm);
    if (base > 0) check(base - 1, d, dm);
    if (base < kTop) check(base + 1, d, dm);
  }
}

}  // namespace

int main() {
  std::vector<uint64_t> divs = {1, 2, 3, 10, 1000000000000000000ull, kTop - 1, kTop};
  for (int k = 1; k <= 62; ++k) {
    divs.push_back(uint64_t(1) << k);
    divs.push_back((uint64_t(1) << k) + 1);
    divs.push_back((uint64_t(1) << k) - 1);
  }
  for (int i = 0; i < 63 * 64; ++i) {   // 4032 random divisors, 64 of every bit length 1..63
    const int bits = 1 + i % 63;
    const uint64_t lo = uint64_t(1) << (bits - 1);
    divs.push_back(lo + (bits > 1 ? rnd() % lo : 0));
  }
  for (uint64_t d : divs) check_divisor(d);
  std::printf("%zu divisors, %lld checks, %lld failures\n", divs.size(), checks, failures);
  return failures ? 1 : 0;
}
