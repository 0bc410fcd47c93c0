// The host plan of pe_fit_explain (csrc/pe_explain_plan.h) on the CPU, stand-alone: built with the address and
// undefined-behaviour sanitizers by tests/test_explain_plan_cpu.py and run directly.  Chunks against an exact cover
// of [0, S), the leaf -> level-domain map against a brute-force walk on random hierarchies, every refusal with its
// index, and the dedupe against a brute-force scan (equal shapes in different domains stay distinct).
#include <cstdio>
#include <random>
#include <vector>

#include "pe_explain_plan.h"

static int g_cases = 0, g_checked = 0, g_fail = 0;

#define CHECK(c)                                                  \
  do {                                                            \
    ++g_checked;                                                  \
    if (!(c)) {                                                   \
      ++g_fail;                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
    }                                                             \
  } while (0)

static void chunks() {
  const int64_t rec = pe::EX_OUT_WORDS * (int64_t)sizeof(uint64_t);
  for (int64_t S : {int64_t(1), int64_t(2), int64_t(7), int64_t(64), int64_t(1000)}) {
    for (int64_t want : {int64_t(1), S - 1, S, S + 1}) {
      if (want < 1) continue;
      for (int64_t slack : {int64_t(0), rec - 1}) {   // a budget of exactly `want` records, and just below one more
        ++g_cases;
        const int64_t chunk = pe::explain_chunk(S, want * rec + slack);
        CHECK(chunk == std::min(S, want));
        std::vector<int> seen((size_t)S, 0);
        int64_t launches = 0;
        for (int64_t s0 = 0; s0 < S; s0 += chunk, ++launches)
          for (int64_t s = s0; s < std::min(S, s0 + chunk); ++s) ++seen[(size_t)s];
        for (int64_t s = 0; s < S; ++s) CHECK(seen[(size_t)s] == 1);
        CHECK(launches == (S + chunk - 1) / chunk);
        CHECK(chunk * rec <= std::max(want * rec + slack, rec));
      }
    }
    ++g_cases;
    CHECK(pe::explain_chunk(S, 0) == 1);            // a budget below one record: one record per launch
    CHECK(pe::explain_chunk(S, pe::EX_BUDGET_BYTES) == std::min<int64_t>(S, pe::EX_BUDGET_BYTES / rec));
  }
  CHECK(pe::EX_BUDGET_BYTES / rec == 233016);       // the seam the GPU suite crosses
}

static void leaf_maps() {
  std::mt19937_64 rng(5);
  for (int it = 0; it < 300; ++it) {
    ++g_cases;
    const int n_levels = 1 + (int)(rng() % 4);
    std::vector<int32_t> size((size_t)n_levels);
    for (int l = 0; l < n_levels; ++l) size[(size_t)l] = 1 + (int32_t)(rng() % (l == 0 ? 40 : 9));
    std::vector<int32_t> parent;
    for (int l = 0; l + 1 < n_levels; ++l)
      for (int32_t k = 0; k < size[(size_t)l]; ++k)
        parent.push_back(rng() % 4 == 0 ? -1 : (int32_t)(rng() % (uint64_t)size[(size_t)l + 1]));
    for (int level = 0; level < n_levels; ++level) {
      std::vector<int32_t> got(3, 77);   // resized by the call
      pe::explain_leaf_dom(level, size.data(), parent.data(), got);
      CHECK((int32_t)got.size() == size[0]);
      for (int32_t k = 0; k < size[0]; ++k) {
        int32_t d = k, off = 0;
        bool none = false;
        for (int l = 0; l < level; ++l) {   // brute force: one step at a time, by the header comment of placement.h
          if (parent[(size_t)(off + d)] < 0) {
            none = true;
            break;
          }
          d = parent[(size_t)(off + d)];
          off += size[(size_t)l];
        }
        CHECK(got[(size_t)k] == (none ? pe::EX_NO_DOMAIN : d));
        CHECK(none || (d >= 0 && d < size[(size_t)level]));
      }
    }
  }
}

static void refusals() {
  pe::TreePlanError te;
  int64_t bad;
  const int64_t req[12] = {1, 2, 3, 4, 0, 0, 0, 0, 5, 6, 7, 8};
  const int32_t size[3] = {4, 2, 1};
  const int32_t parent[6] = {0, 1, -1, 0, 0, 0};
  const int32_t dom[3] = {0, -1, 1};
  ++g_cases;
  CHECK(pe::explain_validate(3, req, nullptr, 9, -3, nullptr, nullptr, &te, &bad) == pe::EX_OK && bad == -1);
  CHECK(pe::explain_validate(3, req, dom, 1, 3, size, parent, &te, &bad) == pe::EX_OK && bad == -1);
  CHECK(pe::explain_validate(0, nullptr, nullptr, 0, 0, nullptr, nullptr, &te, &bad) == pe::EX_OK);
  CHECK(pe::explain_validate(3, nullptr, nullptr, 0, 0, nullptr, nullptr, &te, &bad) == pe::EX_NO_REQ && bad == -1);
  for (int i = 0; i < 12; ++i) {   // a negative request: the first one is named, before anything of the hierarchy
    ++g_cases;
    int64_t r2[12];
    for (int k = 0; k < 12; ++k) r2[k] = k >= i && (k - i) % 5 == 0 ? -1 - k : req[k];
    CHECK(pe::explain_validate(3, r2, dom, 7, 9, nullptr, nullptr, &te, &bad) == pe::EX_BAD_REQ && bad == i);
  }
  ++g_cases;
  CHECK(pe::explain_validate(3, req, dom, 0, 0, size, parent, &te, &bad) == pe::EX_BAD_TREE && te == pe::TREE_BAD_LEVELS);
  CHECK(pe::explain_validate(3, req, dom, 0, 5, size, parent, &te, &bad) == pe::EX_BAD_TREE && te == pe::TREE_BAD_LEVELS);
  CHECK(pe::explain_validate(3, req, dom, 0, 3, nullptr, parent, &te, &bad) == pe::EX_BAD_TREE && te == pe::TREE_NO_SIZES);
  CHECK(pe::explain_validate(3, req, dom, 0, 3, size, nullptr, &te, &bad) == pe::EX_BAD_TREE && te == pe::TREE_NO_PARENT);
  const int32_t size0[3] = {4, 0, 1}, size_big[3] = {4, 65537, 1};
  CHECK(pe::explain_validate(3, req, dom, 0, 3, size0, parent, &te, &bad) == pe::EX_BAD_TREE && te == pe::TREE_BAD_SIZE &&
        bad == 1);
  CHECK(pe::explain_validate(3, req, dom, 0, 3, size_big, parent, &te, &bad) == pe::EX_BAD_TREE &&
        te == pe::TREE_BAD_SIZE && bad == 1);
  for (int i = 0; i < 6; ++i)
    for (int32_t v : {-2, 2, 1}) {   // the level above a leaf has 2 domains, the level above a block 1
      const bool ok = v == 1 && i < 4;
      ++g_cases;
      int32_t p2[6];
      for (int k = 0; k < 6; ++k) p2[k] = k >= i ? v : parent[k];
      const pe::ExplainError e = pe::explain_validate(3, req, dom, 0, 3, size, p2, &te, &bad);
      if (ok) CHECK(e == pe::EX_BAD_TREE && te == pe::TREE_BAD_PARENT && bad == 4);   // 1 is no root
      else CHECK(e == pe::EX_BAD_TREE && te == pe::TREE_BAD_PARENT && bad == i);
    }
  ++g_cases;
  CHECK(pe::explain_validate(3, req, dom, -1, 3, size, parent, &te, &bad) == pe::EX_BAD_LEVEL && bad == -1);
  CHECK(pe::explain_validate(3, req, dom, 3, 3, size, parent, &te, &bad) == pe::EX_BAD_LEVEL && bad == -1);
  CHECK(pe::explain_validate(3, req, dom, 0, 1, size, nullptr, &te, &bad) == pe::EX_OK);   // one level: no parent map
  for (int level = 0; level < 3; ++level)
    for (int i = 0; i < 3; ++i)
      for (int32_t v : {-2, size[level]}) {
        ++g_cases;
        int32_t d2[3];
        for (int k = 0; k < 3; ++k) d2[k] = k >= i ? v : (k == 1 ? -1 : 0);
        CHECK(pe::explain_validate(3, req, d2, level, 3, size, parent, &te, &bad) == pe::EX_BAD_DOMAIN && bad == i);
      }
  ++g_cases;
  const int32_t top[3] = {3, -1, 0};
  CHECK(pe::explain_validate(3, req, top, 0, 3, size, parent, &te, &bad) == pe::EX_OK);
  CHECK(pe::explain_validate(3, req, top, 1, 3, size, parent, &te, &bad) == pe::EX_BAD_DOMAIN && bad == 0);
}

static void dedupe() {
  std::mt19937_64 rng(11);
  std::vector<int32_t> table, of;
  std::vector<pe::ExplainRec> uniq;
  for (int it = 0; it < 200; ++it) {
    ++g_cases;
    const int64_t n = (int64_t)(rng() % 400);
    const bool with_need = it % 3 != 0, with_dom = it % 2 == 0;
    std::vector<int64_t> req((size_t)n * 4);
    std::vector<uint32_t> need((size_t)n);
    std::vector<int32_t> dom((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
      for (int d = 0; d < 4; ++d) req[(size_t)(j * 4 + d)] = (int64_t)(rng() % 2) << (d == 1 ? 62 : 3);
      need[(size_t)j] = (uint32_t)(rng() % 2) << 31;
      dom[(size_t)j] = (int32_t)(rng() % 3) - 1;
      if (j > 0 && rng() % 4 == 0) {   // a run of equal jobs
        for (int d = 0; d < 4; ++d) req[(size_t)(j * 4 + d)] = req[(size_t)((j - 1) * 4 + d)];
        need[(size_t)j] = need[(size_t)j - 1];
        dom[(size_t)j] = dom[(size_t)j - 1];
      }
    }
    const int64_t S = pe::explain_dedupe(n, req.data(), with_need ? need.data() : nullptr,
                                         with_dom ? dom.data() : nullptr, table, of, uniq);
    CHECK(S == (int64_t)uniq.size() && (int64_t)of.size() == n);
    // brute force: first-seen order
    std::vector<pe::ExplainRec> want;
    for (int64_t j = 0; j < n; ++j) {
      pe::ExplainRec r{};
      for (int d = 0; d < 4; ++d) r.q[d] = req[(size_t)(j * 4 + d)];
      r.need = with_need ? need[(size_t)j] : 0u;
      r.dom = with_dom ? dom[(size_t)j] : pe::EX_ANY;
      size_t u = 0;
      for (; u < want.size(); ++u)
        if (want[u].q[0] == r.q[0] && want[u].q[1] == r.q[1] && want[u].q[2] == r.q[2] && want[u].q[3] == r.q[3] &&
            want[u].need == r.need && want[u].dom == r.dom)
          break;
      if (u == want.size()) want.push_back(r);
      CHECK(of[(size_t)j] == (int32_t)u);
    }
    CHECK(want.size() == uniq.size());
    for (size_t u = 0; u < want.size() && u < uniq.size(); ++u) {
      CHECK(uniq[u].need == want[u].need && uniq[u].dom == want[u].dom);
      for (int d = 0; d < 4; ++d) CHECK(uniq[u].q[d] == want[u].q[d]);
      for (uint32_t p : uniq[u].pad_) CHECK(p == 0);
    }
  }
  // one shape in three domains: three records
  ++g_cases;
  const int64_t req[12] = {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4};
  const uint32_t need[3] = {5, 5, 5};
  const int32_t dom[3] = {0, 1, -1};
  CHECK(pe::explain_dedupe(3, req, need, dom, table, of, uniq) == 3 && of[0] == 0 && of[1] == 1 && of[2] == 2);
  CHECK(pe::explain_dedupe(3, req, need, nullptr, table, of, uniq) == 1 && of[2] == 0 && uniq[0].dom == pe::EX_ANY);
  CHECK(pe::explain_dedupe(0, nullptr, nullptr, nullptr, table, of, uniq) == 0 && of.empty() && uniq.empty());
}

int main() {
  chunks();
  leaf_maps();
  refusals();
  dedupe();
  std::printf("%d cases, %d checks, %d failures\n", g_cases, g_checked, g_fail);
  return g_fail ? 1 : 0;
}
