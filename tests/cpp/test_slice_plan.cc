// pe_slice_plan.h on the host, stand-alone (built with -fsanitize=address,undefined by
// tests/test_slice_plan_cpu.py): each refusal with its index, the rows and picks of random batches against a
// brute-force scan, the canonical row of z = 1, and the unit conversion at its corners.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "pe_slice_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                             \
    }                                                         \
  } while (0)

static void refusals() {
  const int n = 6, L = 3;
  const std::vector<int32_t> count{8, 16, 24, 8, 8, 6}, z{8, 8, 8, 4, 2, 3}, sl{-1, 0, 1, 2, 0, -1}, ml{2, 2, 2, 2, 0, 1};
  int64_t bad = -1;
  CHECK(pe::slice_validate(n, count.data(), z.data(), sl.data(), ml.data(), L, &bad) == pe::SLICE_OK && bad == -1);
  CHECK(pe::slice_validate(n, count.data(), nullptr, nullptr, nullptr, L, &bad) == pe::SLICE_OK);
  CHECK(pe::slice_validate(0, nullptr, nullptr, nullptr, nullptr, L, &bad) == pe::SLICE_OK);
  for (int32_t v : {0, -1, INT32_MIN}) {
    auto b = z;
    b[2] = v;
    b[4] = 0;
    CHECK(pe::slice_validate(n, count.data(), b.data(), sl.data(), ml.data(), L, &bad) == pe::SLICE_BAD_SIZE && bad == 2);
  }
  {   // a bad size further on wins over an earlier count that is no multiple: the checks run one after the other
    auto b = z;
    auto c = count;
    c[1] = 17;
    b[5] = 0;
    CHECK(pe::slice_validate(n, c.data(), b.data(), sl.data(), ml.data(), L, &bad) == pe::SLICE_BAD_SIZE && bad == 5);
    CHECK(pe::slice_validate(n, c.data(), z.data(), sl.data(), ml.data(), L, &bad) == pe::SLICE_BAD_COUNT && bad == 1);
    CHECK(pe::slice_validate(n, c.data(), nullptr, sl.data(), ml.data(), L, &bad) == pe::SLICE_OK);   // z = 1
  }
  for (int32_t v : {-2, L, INT32_MAX, INT32_MIN}) {
    auto b = sl;
    b[3] = v;
    b[5] = L;
    CHECK(pe::slice_validate(n, count.data(), z.data(), b.data(), ml.data(), L, &bad) == pe::SLICE_BAD_LEVEL && bad == 3);
  }
  {
    auto b = ml;
    b[3] = 1;   // sl = 2
    CHECK(pe::slice_validate(n, count.data(), z.data(), sl.data(), b.data(), L, &bad) == pe::SLICE_BAD_MAX_LEVEL && bad == 3);
    b = ml;
    b[2] = 0;   // sl = 1
    CHECK(pe::slice_validate(n, count.data(), z.data(), sl.data(), b.data(), L, &bad) == pe::SLICE_BAD_MAX_LEVEL && bad == 2);
    // max_level 0 is enough for node level and level 0; the default is the top level
    std::vector<int32_t> zero(n, 0), low{-1, 0, -1, 0, 0, -1};
    CHECK(pe::slice_validate(n, count.data(), z.data(), low.data(), zero.data(), L, &bad) == pe::SLICE_OK);
    CHECK(pe::slice_validate(n, count.data(), z.data(), sl.data(), nullptr, L, &bad) == pe::SLICE_OK);
    CHECK(pe::slice_validate(n, count.data(), z.data(), sl.data(), nullptr, 2, &bad) == pe::SLICE_BAD_LEVEL && bad == 3);
  }
}

static void conversion() {
  const uint64_t cap_max = 2147483647ull;   // PE_CAP_MAX
  for (uint32_t z : {1u, 2u, 3u, 8u, 64u, 2147483647u}) {
    CHECK(pe::slice_units(0, z) == 0);
    CHECK(pe::slice_units(z - 1, z) == 0);
    CHECK(pe::slice_units(z, z) == 1);
    CHECK(pe::slice_units(cap_max, z) == cap_max / z);
    CHECK(pe::slice_units((uint64_t(1) << 55) - 1, z) == ((uint64_t(1) << 55) - 1) / z);
    CHECK(pe::slice_units(2ull * z - 1, z) == 1 && pe::slice_units(2ull * z, z) == 2);
  }
  CHECK(pe::slice_units(cap_max, 2147483647u) == 1 && pe::slice_units(cap_max - 1, 2147483647u) == 0);
  // the canonical row: z = 1 names the same row at node level and at level 0, and nothing else is folded
  CHECK(pe::slice_row(5, 1, -1) == pe::slice_row(5, 1, 0) && pe::slice_row(5, 1, -1).sl == 0);
  CHECK(!(pe::slice_row(5, 1, 1) == pe::slice_row(5, 1, 0)) && !(pe::slice_row(5, 2, -1) == pe::slice_row(5, 2, 0)));
  CHECK(pe::slice_row(5, 2, -1).sl == -1 && pe::slice_floor(-1) == 0 && pe::slice_floor(0) == 0 && pe::slice_floor(3) == 3);
  const uint64_t k = pe::slice_pick_key(2147483646u, 2147483647, 3);
  CHECK(pe::slice_pick_row(k) == 2147483646u && pe::slice_pick_units(k) == 2147483647 && pe::slice_pick_max_level(k) == 3);
}

// rows and picks of a batch by a scan over everything seen so far
static int64_t batches(int n_batches) {
  static const int32_t kSizes[5] = {1, 1, 2, 3, 8};
  std::mt19937_64 rng(23);
  pe::SlicePlan plan;
  int64_t jobs = 0;
  for (int b = 0; b < n_batches; ++b) {
    const int n = (int)(rng() % 200), L = 1 + (int)(rng() % 4);
    const bool has_z = rng() % 8 != 0, has_sl = rng() % 8 != 0, has_ml = rng() % 4 != 0;
    std::vector<int32_t> shape(n), count(n), z(n), sl(n), ml(n);
    for (int j = 0; j < n; ++j) {
      if (j > 0 && rng() % 4 == 0) {   // runs of equal jobs
        shape[j] = shape[j - 1], count[j] = count[j - 1], z[j] = z[j - 1], sl[j] = sl[j - 1], ml[j] = ml[j - 1];
        continue;
      }
      shape[j] = (int32_t)(rng() % 5);
      z[j] = has_z ? kSizes[rng() % 5] : 1;
      sl[j] = has_sl ? (int32_t)(rng() % (L + 1)) - 1 : 0;
      count[j] = z[j] * (1 + (int32_t)(rng() % 4));
      ml[j] = has_ml ? pe::slice_floor(sl[j]) + (int32_t)(rng() % (L - pe::slice_floor(sl[j]))) : L - 1;
    }
    pe::slice_plan_build(plan, n, shape.data(), count.data(), has_z ? z.data() : nullptr, has_sl ? sl.data() : nullptr,
                         has_ml ? ml.data() : nullptr, L);
    std::vector<pe::SliceRow> rows;
    std::vector<uint64_t> picks;
    CHECK((int)plan.row_of.size() == n && (int)plan.pick_of.size() == n);
    for (int j = 0; j < n; ++j) {
      pe::SliceRow r{(uint32_t)shape[j], z[j], (z[j] == 1 && sl[j] == -1) ? 0 : sl[j], 0};
      size_t at = 0;
      while (at < rows.size() && !(rows[at] == r)) ++at;
      if (at == rows.size()) rows.push_back(r);
      CHECK(plan.row_of[j] == (int32_t)at);
      const uint64_t key = ((uint64_t)at << 33) | ((uint64_t)(count[j] / z[j]) << 2) | (uint64_t)ml[j];
      size_t pt = 0;
      while (pt < picks.size() && picks[pt] != key) ++pt;
      if (pt == picks.size()) picks.push_back(key);
      CHECK(plan.pick_of[j] == (int32_t)pt);
    }
    CHECK(plan.rows.size() == rows.size() && plan.picks == picks);
    for (size_t r = 0; r < rows.size() && r < plan.rows.size(); ++r) CHECK(plan.rows[r] == rows[r] && plan.rows[r].pad_ == 0);
    jobs += n;
  }
  return jobs;
}

int main() {
  refusals();
  conversion();
  const int n_batches = 400;
  const int64_t jobs = batches(n_batches);
  std::printf("%d batches, %lld jobs checked, %d failures\n", n_batches, (long long)jobs, failures);
  return failures ? 1 : 0;
}
