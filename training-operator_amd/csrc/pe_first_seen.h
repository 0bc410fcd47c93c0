// First-seen dedupe: the distinct keys of n items numbered in the order of their first appearance, and each
// item's number.  The gang-capacity calls (pe_engine_capacity.cpp) reduce a batch to its distinct pod
// shapes and its distinct (shape, count, max_level) picks with it; the order is part of their contract
// (the chunk of device tables a shape lands in follows from its number).  Plain C++, no HIP:
// tests/cpp/test_first_seen.cc runs it under the sanitizers against a brute-force scan.
//
// The caller owns the keys: the header sees items and distinct keys by index only.
//   hash(j)     a 64-bit hash of item j's key (its low bits index the table: see first_seen_mix)
//   same(j, u)  item j's key equals distinct key u (u < the number reported so far)
//   add(j)      item j's key is new: the caller appends it as the next distinct key
// Open addressing over a power-of-two table of at least 2 n places (16 at least); an item whose key equals
// its predecessor's skips the probe (batches arrive in runs of equal jobs).  `table` and `index_of` are the
// caller's and keep their storage between calls: nothing is allocated once they have grown.
#ifndef PE_FIRST_SEEN_H_
#define PE_FIRST_SEEN_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pe {

// The finishing step of the key hashes: multiply, then fold the high bits down to where the table index is.
inline uint64_t first_seen_mix(uint64_t h) {
  h *= 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}

// index_of[j] = the number of item j's key (j < n); returns the number of distinct keys (< 2^31: n is).
template <class Hash, class Same, class Add>
int64_t first_seen(int64_t n, std::vector<int32_t>& table, std::vector<int32_t>& index_of, Hash hash, Same same,
                   Add add) {
  index_of.resize((size_t)(n > 0 ? n : 0));
  size_t cap = 16;
  while (cap < (size_t)(n > 0 ? n : 0) * 2) cap <<= 1;
  table.assign(cap, -1);
  int32_t distinct = 0;
  for (int64_t j = 0; j < n; ++j) {
    if (j > 0 && same(j, index_of[(size_t)j - 1])) {
      index_of[(size_t)j] = index_of[(size_t)j - 1];
      continue;
    }
    size_t at = (size_t)hash(j) & (cap - 1);
    while (table[at] >= 0 && !same(j, table[at])) at = (at + 1) & (cap - 1);   // ends: half the places are free
    if (table[at] < 0) {
      table[at] = distinct++;
      add(j);
    }
    index_of[(size_t)j] = table[at];
  }
  return distinct;
}

}  // namespace pe

#endif  // PE_FIRST_SEEN_H_
