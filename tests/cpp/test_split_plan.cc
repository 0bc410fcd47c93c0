// csrc/pe_split_plan.h on the CPU, stand-alone (tests/test_split_plan_cpu.py builds it with the address and
// undefined-behaviour sanitizers): split_tr against a brute-force walk over sorted children, its extremes,
// the slice rule at the 64 MiB boundary, the copy ranges and the scatter from picks to jobs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "pe_split_plan.h"

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      ++failures;                                               \
    }                                                           \
  } while (0)

using Parts = std::vector<std::pair<int, uint64_t>>;

// include/placement.h's walk: children by (slots descending, id ascending), whole parts while slots < r,
// the last part to the smallest slots >= r among the rest, ties to the smallest id
static Parts walk(const std::vector<uint64_t>& sl, uint64_t a) {
  std::vector<int> order(sl.size());
  for (size_t i = 0; i < sl.size(); ++i) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sl[(size_t)x] > sl[(size_t)y]; });
  Parts out;
  uint64_t r = a;
  for (size_t pos = 0; pos < order.size(); ++pos) {
    const int i = order[pos];
    if (sl[(size_t)i] >= r) {
      int best = -1;
      for (size_t q = pos; q < order.size(); ++q) {
        const int x = order[q];
        if (sl[(size_t)x] < r) continue;
        if (best < 0 || sl[(size_t)x] < sl[(size_t)best] || (sl[(size_t)x] == sl[(size_t)best] && x < best)) best = x;
      }
      out.push_back({best, r});
      return out;
    }
    out.push_back({i, sl[(size_t)i]});
    r -= sl[(size_t)i];
  }
  return {};
}

// the threshold form on top of split_tr, as tree_split_kernel applies it
static Parts threshold(const std::vector<uint64_t>& sl, uint64_t a) {
  uint64_t v = 0;
  for (uint64_t c : sl) {   // the largest child value with H >= a
    uint64_t h = 0;
    for (uint64_t x : sl) h += x >= c ? x : 0;
    if (c > 0 && h >= a && c > v) v = c;
  }
  uint64_t G = 0;
  for (uint64_t x : sl) G += x > v ? x : 0;
  const pe::SplitTR tr = pe::split_tr(a, G, v);
  CHECK(tr.r > 0 && tr.r <= v);
  Parts whole;
  uint64_t eq = 0;
  std::vector<char> taken(sl.size(), 0);
  for (size_t i = 0; i < sl.size(); ++i) {
    const bool w = sl[i] > v || (sl[i] == v && eq < tr.t);
    eq += sl[i] == v ? 1 : 0;
    if (w) {
      whole.push_back({(int)i, sl[i]});
      taken[i] = 1;
    }
  }
  std::stable_sort(whole.begin(), whole.end(),
                   [](const std::pair<int, uint64_t>& x, const std::pair<int, uint64_t>& y) { return x.second > y.second; });
  int best = -1;
  for (size_t i = 0; i < sl.size(); ++i)
    if (!taken[i] && sl[i] >= tr.r && (best < 0 || sl[i] < sl[(size_t)best])) best = (int)i;
  whole.push_back({best, tr.r});
  return whole;
}

int main() {
  std::mt19937_64 rng(21);
  const uint64_t menu[] = {0, 0, 1, 2, 3, 5, 5, 8, 13};
  int lists = 0;
  int64_t steps = 0;
  while (lists < 300) {
    const size_t n = 1 + rng() % 12;
    std::vector<uint64_t> sl(n);
    uint64_t sum = 0;
    for (auto& x : sl) sum += x = menu[rng() % 9];
    if (sum == 0) continue;
    ++lists;
    for (uint64_t a = 1; a <= sum; ++a, ++steps) {   // every allotment the parent can get
      const Parts w = walk(sl, a), t = threshold(sl, a);
      CHECK(!w.empty() && w == t);
      uint64_t pods = 0;
      for (const auto& p : w) {
        pods += p.second;
        CHECK(p.first >= 0 && p.second >= 1 && p.second <= sl[(size_t)p.first]);
      }
      CHECK(pods == a);
    }
  }
  // hand-made traps
  CHECK((walk({10, 7, 6, 3}, 13) == Parts{{0, 10}, {3, 3}}) && (threshold({10, 7, 6, 3}, 13) == Parts{{0, 10}, {3, 3}}));
  CHECK((threshold({5, 5, 5, 5}, 12) == Parts{{0, 5}, {1, 5}, {2, 2}}));
  CHECK((threshold({8, 4, 4}, 12) == Parts{{0, 8}, {1, 4}}));
  CHECK((threshold({10, 7, 3}, 3) == Parts{{2, 3}}));
  // the extremes: values near 2^55 (the tables' bound) and the largest count
  const uint64_t big = (uint64_t(1) << 55) - 1, top = (uint64_t(1) << 31) - 1;
  pe::SplitTR tr = pe::split_tr(top, 0, big);
  CHECK(tr.t == 0 && tr.r == top);
  tr = pe::split_tr(big, 0, big);
  CHECK(tr.t == 0 && tr.r == big);
  tr = pe::split_tr(3 * big, big, big);   // 2 * big left for children of big slots: one whole, the last one full
  CHECK(tr.t == 1 && tr.r == big);
  tr = pe::split_tr(3 * big - 1, big, big);
  CHECK(tr.t == 1 && tr.r == big - 1);
  tr = pe::split_tr(top, 0, 1);
  CHECK(tr.t == top - 1 && tr.r == 1);
  tr = pe::split_tr(top, 7, 1000);
  CHECK(tr.t == (top - 7 - 1) / 1000 && tr.r == top - 7 - tr.t * 1000 && tr.r >= 1 && tr.r <= 1000);
  tr = pe::split_tr(1, 0, 1);
  CHECK(tr.t == 0 && tr.r == 1);
  // slices: the most picks whose rows stay within 64 MiB, for the narrowest, a middle and the widest row
  for (int32_t mp : {1, 64, 1024}) {
    const int64_t n = pe::split_slice_picks(mp);
    CHECK(pe::split_row_bytes(mp) == 8 * (int64_t)mp + 20);
    CHECK(n >= 1 && n * pe::split_row_bytes(mp) <= pe::SPLIT_BUFFER_BYTES);
    CHECK((n + 1) * pe::split_row_bytes(mp) > pe::SPLIT_BUFFER_BYTES);
    const pe::SplitLayout L{n, mp};
    CHECK(L.words() * 4 == n * pe::split_row_bytes(mp) && L.words() * 4 <= pe::SPLIT_BUFFER_BYTES);
    CHECK(L.dom_at() == 0 && L.meta_at() == n * mp && L.pods_at() == n * mp + 5 * n);
  }
  CHECK(pe::split_slice_picks(1) == 2396745 && pe::split_slice_picks(64) == 126144 && pe::split_slice_picks(1024) == 8172);
  // copy ranges: one contiguous range for every subset of the three blocks, never more than it has to be
  {
    const pe::SplitLayout L{7, 3};
    for (int m = 0; m < 8; ++m) {
      const bool dom = m & 1, meta = m & 2, pods = m & 4;
      const pe::SplitRange r = pe::split_copy_range(L, dom, meta, pods);
      if (m == 0) {
        CHECK(r.count == 0);
        continue;
      }
      if (dom) CHECK(r.first <= L.dom_at() && r.first + r.count >= L.meta_at());
      if (meta) CHECK(r.first <= L.meta_at() && r.first + r.count >= L.pods_at());
      if (pods) CHECK(r.first <= L.pods_at() && r.first + r.count >= L.words());
      CHECK(r.first >= 0 && r.first + r.count <= L.words());
      if (!dom) CHECK(r.first >= L.meta_at());
      if (!dom && !meta) CHECK(r.first == L.pods_at());
      if (!pods) CHECK(r.first + r.count <= L.pods_at());
      if (!pods && !meta) CHECK(r.first + r.count == L.meta_at());
    }
  }
  // the scatter: a slice [p0, p0 + n) of the picks, some of them not answered by this launch, to 40 jobs
  {
    const int32_t mp = 3, levels = 3;
    const int64_t p0 = 5, n = 6, J = 40;
    const pe::SplitLayout L{n, mp};
    std::vector<int32_t> buf((size_t)L.words());
    for (int64_t k = 0; k < n; ++k) {
      for (int i = 0; i < mp; ++i) {
        buf[(size_t)(L.dom_at() + k * mp + i)] = (int32_t)(1000 + 10 * k + i);
        buf[(size_t)(L.pods_at() + k * mp + i)] = (int32_t)(2000 + 10 * k + i);
      }
      buf[(size_t)(L.meta_at() + k * 5)] = (int32_t)(k % 4);
      for (int l = 0; l < 4; ++l) buf[(size_t)(L.meta_at() + k * 5 + 1 + l)] = (int32_t)(3000 + 10 * k + l);
    }
    std::vector<int32_t> pick_of((size_t)J);
    for (int64_t j = 0; j < J; ++j) pick_of[(size_t)j] = (int32_t)(rng() % 14);
    auto live = [](int64_t p) { return p != 7; };
    for (int m = 1; m < 16; ++m) {
      std::vector<int32_t> parts((size_t)J, -9), dom((size_t)(J * mp), -9), pods((size_t)(J * mp), -9),
          spread((size_t)(J * levels), -9);
      for (int64_t j0 : {int64_t(0), int64_t(13)})   // two ranges of jobs, as two threads would take them
        pe::split_scatter(buf.data(), L, p0, j0, j0 ? J : 13, pick_of.data(), levels, live, m & 1 ? parts.data() : nullptr,
                          m & 2 ? dom.data() : nullptr, m & 4 ? pods.data() : nullptr, m & 8 ? spread.data() : nullptr);
      for (int64_t j = 0; j < J; ++j) {
        const int64_t p = pick_of[(size_t)j], k = p - p0;
        const bool hit = k >= 0 && k < n && p != 7;
        CHECK(parts[(size_t)j] == (hit && (m & 1) ? (int32_t)(k % 4) : -9));
        for (int i = 0; i < mp; ++i) {
          CHECK(dom[(size_t)(j * mp + i)] == (hit && (m & 2) ? (int32_t)(1000 + 10 * k + i) : -9));
          CHECK(pods[(size_t)(j * mp + i)] == (hit && (m & 4) ? (int32_t)(2000 + 10 * k + i) : -9));
        }
        for (int l = 0; l < levels; ++l)
          CHECK(spread[(size_t)(j * levels + l)] == (hit && (m & 8) ? (int32_t)(3000 + 10 * k + l) : -9));
      }
    }
  }
  std::printf("%d lists, %lld steps checked, %d failures\n", lists, (long long)steps, failures);
  return failures ? 1 : 0;
}
