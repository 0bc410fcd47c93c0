// The first-seen dedupe of the gang-capacity calls (training-operator_amd/csrc/pe_first_seen.h) against a
// brute-force first-seen scan: the number of each item's key, the distinct keys in the order of their first
// appearance, and what the header asks of its callables.  Built and run by tests/test_first_seen_cpu.py
// with g++ and the address and undefined-behaviour sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_first_seen.h"

static int failed = 0;
static long cases = 0, items_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

enum HashKind { MIXED, IDENTITY, CONSTANT };

// The table storage, kept across cases as the engine keeps it across calls.
static std::vector<int32_t> table, index_of;

// first_seen over `keys` with the given hash against the scan that compares every item with every distinct
// key so far.  Returns the number of hash probes skipped by the predecessor shortcut.
static long verify(const char* name, const std::vector<uint64_t>& keys, HashKind kind) {
  const int64_t n = (int64_t)keys.size();
  std::vector<uint64_t> want_keys;
  std::vector<int32_t> want_of;
  for (int64_t j = 0; j < n; ++j) {
    size_t u = 0;
    while (u < want_keys.size() && want_keys[u] != keys[(size_t)j]) ++u;
    if (u == want_keys.size()) want_keys.push_back(keys[(size_t)j]);
    want_of.push_back((int32_t)u);
  }
  std::vector<uint64_t> got_keys;
  long hashed = 0;
  bool in_range = true, new_is_new = true;
  const int64_t got = pe::first_seen(
      n, table, index_of,
      [&](int64_t j) {
        ++hashed;
        in_range &= j >= 0 && j < n;
        const uint64_t k = keys[(size_t)j];
        return kind == MIXED ? pe::first_seen_mix(k) : kind == IDENTITY ? k : uint64_t(5);
      },
      [&](int64_t j, int32_t u) {
        in_range &= j >= 0 && j < n && u >= 0 && (size_t)u < got_keys.size();
        return got_keys[(size_t)u] == keys[(size_t)j];
      },
      [&](int64_t j) {
        in_range &= j >= 0 && j < n;
        new_is_new &= std::find(got_keys.begin(), got_keys.end(), keys[(size_t)j]) == got_keys.end();
        got_keys.push_back(keys[(size_t)j]);
      });
  ++cases;
  items_checked += n;
  check(name, in_range && new_is_new);
  check(name, got == (int64_t)want_keys.size() && got_keys == want_keys);
  check(name, (int64_t)index_of.size() == n && std::equal(want_of.begin(), want_of.end(), index_of.begin()));
  // the table: a power of two, at least 16 and at least 2 n places; every distinct key in it once
  const size_t cap = table.size();
  check(name, cap >= 16 && (cap & (cap - 1)) == 0 && cap >= (size_t)n * 2);
  std::vector<int32_t> held;
  for (int32_t v : table)
    if (v >= 0) held.push_back(v);
  std::sort(held.begin(), held.end());
  bool dense = held.size() == want_keys.size();
  for (size_t u = 0; dense && u < held.size(); ++u) dense = held[u] == (int32_t)u;
  check(name, dense);
  check(name, hashed <= n);
  return (long)n - hashed;
}

int main() {
  std::mt19937_64 rng(11);
  const HashKind kinds[3] = {MIXED, IDENTITY, CONSTANT};
  const int sizes[] = {0, 1, 2, 15, 16, 17, 3000};
  for (HashKind kind : kinds)
    for (int n : sizes) {
      if (kind == CONSTANT && n > 17) n = 600;   // every key in one probe chain: quadratic
      std::vector<uint64_t> keys((size_t)n);
      // all keys equal: one key, and every item but the first takes the shortcut
      std::fill(keys.begin(), keys.end(), uint64_t(42));
      check("all equal: shortcut", verify("all equal", keys, kind) == std::max(0, n - 1));
      // all keys distinct
      for (int j = 0; j < n; ++j) keys[(size_t)j] = (uint64_t)j * 7919 + 3;
      check("all distinct: no shortcut", verify("all distinct", keys, kind) == 0);
      // long runs of equal keys, the runs' keys recurring
      for (int j = 0; j < n; ++j) keys[(size_t)j] = (uint64_t)((j / 50) % 9);
      const long skipped = verify("runs", keys, kind);
      check("runs: shortcut", skipped == n - (n + 49) / 50);
      // keys that recur out of order
      for (int j = 0; j < n; ++j) keys[(size_t)j] = rng() % (uint64_t)(n / 3 + 1);
      verify("out of order", keys, kind);
      // keys that share the low bits of the table index: multiples of a power of two above the table's
      // size, under the identity hash all in one probe chain
      for (int j = 0; j < n; ++j) keys[(size_t)j] = (rng() % (uint64_t)(n / 2 + 1)) << 20;
      verify("low bits collide", keys, kind);
      // keys that differ in the high bits only
      for (int j = 0; j < n; ++j) keys[(size_t)j] = (rng() % 5) << 61;
      verify("high bits", keys, kind);
    }
  // a second call that reuses the table storage with a smaller n: nothing of the first call is seen
  {
    std::vector<uint64_t> big(5000), small_keys = {9, 9, 4, 9, 4, 7};
    for (size_t j = 0; j < big.size(); ++j) big[j] = j % 1234;
    verify("large first", big, MIXED);
    const size_t big_cap = table.capacity(), big_of = index_of.capacity();
    verify("smaller second", small_keys, MIXED);
    check("smaller second: table shrinks to 16 places", table.size() == 16);
    check("smaller second: storage kept", table.capacity() == big_cap && index_of.capacity() == big_of);
    check("smaller second: numbers", index_of == std::vector<int32_t>({0, 0, 1, 0, 1, 2}));
    verify("empty third", {}, MIXED);
    check("empty third: storage kept", table.capacity() == big_cap && index_of.empty());
    verify("large again", big, IDENTITY);
    check("large again: no growth", table.capacity() == big_cap && index_of.capacity() == big_of);
  }
  // random batches: sizes around the table's growth steps, few or many distinct keys
  for (int it = 0; it < 200; ++it) {
    const int n = (int)(rng() % 70);
    const uint64_t span = 1 + rng() % (it % 2 ? 6 : 200);
    std::vector<uint64_t> keys((size_t)n);
    for (auto& k : keys) k = (rng() % span) * (it % 3 == 0 ? 64 : 1);
    verify("random", keys, kinds[it % 3]);
  }
  printf("%ld cases, %ld items checked, %d failures\n", cases, items_checked, failed);
  return failed ? 1 : 0;
}
