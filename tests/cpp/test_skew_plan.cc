// The plan of pe_place_skew_domains (training-operator_amd/csrc/pe_skew_plan.h): the book of existing pods against a
// brute force on hand-made hierarchies at every (level, spread_level) pair, the skews, the scratch layout, and every
// refusal, each leaving the plan as it was.  Stand-alone; tests/test_skew_plan_cpu.py builds and runs it.
#include <stdio.h>

#include <map>

#include "pe_skew_plan.h"

using pe::SkewPlan;
typedef std::vector<int32_t> Vec;
static int failed = 0;
static long plans = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) failed += printf("FAIL %s\n", name) > 0;
}

// Domain k of level `from`, walked up to level `to` one step at a time.
static int32_t walk(const Vec& sizes, const Vec& parent, int32_t k, int from, int to) {
  int32_t off = 0;
  for (int l = 0; l < from; ++l) off += sizes[(size_t)l];
  for (int l = from; l < to && k >= 0; off += sizes[(size_t)l++]) k = parent[(size_t)(off + k)];
  return k;
}

// Every (level, spread_level, job domain d): two groups' books name every key twice, and once descending.  N = 9.
static void verify(const char* name, const Vec& sizes, const Vec& parent) {
  const int32_t off[2] = {0, 2}, pri[1] = {0}, cnt[2] = {4, 1}, skews[2] = {3, pe::SKEW_NONE}, N = 9;
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level)
    for (int32_t sl = -1; sl < level; ++sl)
      for (int32_t d = 0; d < sizes[(size_t)level]; ++d) {
        const int32_t K = sl < 0 ? N : sizes[(size_t)sl];
        Vec boff = {0, 2 * K, 3 * K}, bdom, bcnt;
        for (int32_t k = 0; k < 2 * K; ++k) bdom.push_back(k % K), bcnt.push_back(k + 1);
        for (int32_t k = K - 1; k >= 0; --k) bdom.push_back(k), bcnt.push_back(k == 0 ? INT32_MAX : 7);
        SkewPlan p;
        check(name, pe::skew_plan_build(p, 1, off, pri, cnt, skews, sl, boff.data(), bdom.data(), bcnt.data(), sl & 1, &d, level,
                                        (int32_t)sizes.size(), sizes.data(), parent.data(), N) == pe::SKEW_OK);
        ++plans;
        check(name, p.by_node() == (sl < 0) && p.dry_run == ((sl & 1) != 0) && p.skew == Vec({3, pe::SKEW_FREE}) &&
                        p.constrained() && p.n_keys == K && p.book_off.size() == 3 && p.book_off[0] == 0);
        for (int g = 0; g < 2; ++g) {   // brute force: the keys under d, ascending, their counts added up
          std::map<int32_t, int64_t> want;
          for (int32_t e = boff[(size_t)g]; e < boff[(size_t)g + 1]; ++e)
            if (sl < 0 || walk(sizes, parent, bdom[(size_t)e], sl, level) == d) want[bdom[(size_t)e]] += bcnt[(size_t)e];
          size_t at = (size_t)p.book_off[(size_t)g];
          check(name, (size_t)p.book_off[(size_t)g + 1] == at + want.size());
          for (auto kv = want.begin(); kv != want.end(); ++kv, ++at)
            check(name, at < p.book.size() && p.book[at].key == kv->first && p.book[at].count == std::min<int64_t>(kv->second, INT32_MAX));
        }
      }
}

int main() {
  verify("regular", {6, 3, 1}, {0, 0, 1, 1, 2, 2, 0, 0, 0});   // four hand-made hierarchies
  verify("orphans", {6, 3, 2}, {0, -1, 1, 1, 2, 0, 1, -1, 1});
  verify("interleaved", {7, 4, 2}, {3, 0, 2, 1, 3, 0, 2, 1, 0, 1, 0});
  verify("four levels", {8, 4, 2, 1}, {0, 1, 2, 3, 3, 2, 1, 0, 1, 0, 1, -1, 0, 0});
  check("scratch", pe::skew_scratch_layout(1018, 77).where_at == 2040 && pe::skew_scratch_layout(1018, 77).words == 2117);
  // ---- refusals, in the order of the checks; the plan stays as it was
  const int32_t off[3] = {0, 1, 3}, pri[2] = {0, 1}, cnt[3] = {2, 1, 3}, dom[2] = {1, 0}, skews[3] = {1, -1, 2};
  const int32_t sizes[3] = {6, 3, 1}, parent[9] = {0, 0, 1, 1, 2, 2, 0, 0, 0};
  const int32_t boff[4] = {0, 1, 1, 3}, bdom[3] = {2, 0, 0}, bcnt[3] = {1, 0, 2};
  SkewPlan p;
  check("a plan to keep", pe::skew_plan_build(p, 2, off, pri, cnt, skews, 0, boff, bdom, bcnt, 0, dom, 1, 3, sizes, parent, 9) == pe::SKEW_OK &&
                              p.skew == Vec({1, 0, 2}) && p.book_off == Vec({0, 1, 1, 2}) && p.book[0].key == 2 && p.book[1].key == 0 && p.book[1].count == 2);
  const SkewPlan before = p;
  auto refused = [&](const char* name, const int32_t* s, int32_t sl, const int32_t* bo, const int32_t* bd, const int32_t* bc,
                     uint32_t flags, const int32_t* d, int32_t level, const int32_t* par, pe::SkewPlanError want,
                     int64_t want_index, pe::PlacePlanError want_place = pe::PLACE_OK) {
    int64_t bad = 99;
    pe::PlacePlanError pe_ = pe::PLACE_OK;
    pe::TreePlanError te = pe::TREE_OK;
    const pe::SkewPlanError e = pe::skew_plan_build(p, 2, off, pri, cnt, s, sl, bo, bd, bc, flags, d, level, 3, sizes, par, 9, &pe_, &te, &bad);
    check(name, e == want && bad == want_index && pe_ == want_place && p.skew == before.skew && p.book_off == before.book_off &&
                    p.book.size() == before.book.size() && p.dry_run == before.dry_run && p.n_keys == before.n_keys &&
                    p.sp.leaf_sd == before.sp.leaf_sd && p.sp.base.jobs == before.sp.base.jobs);
    ++refusals;
  };
  const int32_t d_hi[2] = {1, 3}, zero[3] = {1, 0, 2}, low[3] = {-2, 0, 2}, desc[4] = {0, 2, 1, 3}, neg[4] = {-1, 1, 1, 3};
  const int32_t d_out[3] = {2, 6, -1}, d_neg[3] = {-1, 0, 0}, n_out[3] = {8, 9, 0}, c_neg[3] = {1, 0, -1};
  refused("the hierarchy first", zero, 5, desc, d_out, c_neg, 2, dom, 1, nullptr, pe::SKEW_BAD_PLACE, -1, pe::PLACE_BAD_TREE);
  refused("level", skews, 0, boff, bdom, bcnt, 0, dom, 3, parent, pe::SKEW_BAD_PLACE, -1, pe::PLACE_BAD_LEVEL);
  refused("job_domain", zero, 1, desc, d_out, c_neg, 2, d_hi, 1, parent, pe::SKEW_BAD_PLACE, 1, pe::PLACE_BAD_DOMAIN);
  refused("spread_level -2", zero, -2, desc, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_LEVEL, -1);
  refused("spread_level = level", zero, 1, desc, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_LEVEL, -1);
  refused("skew 0", zero, 0, desc, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_SKEW, 1);
  refused("skew -2", low, -1, desc, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_SKEW, 0);
  refused("offsets descending", skews, 0, desc, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_OFF, 2);
  refused("offsets negative", skews, 0, neg, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_OFF, 0);
  refused("entries without counts", skews, 0, boff, bdom, nullptr, 2, dom, 1, parent, pe::SKEW_BAD_OFF, -1);
  refused("domain outside its level", skews, 0, boff, d_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_DOM, 1);
  refused("node outside [0, N)", skews, -1, boff, n_out, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_DOM, 1);
  refused("negative domain", skews, 0, boff, d_neg, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_DOM, 0);
  refused("negative count", skews, 0, boff, bdom, c_neg, 2, dom, 1, parent, pe::SKEW_BAD_COUNT, 2);
  refused("flags 2", skews, 0, boff, bdom, bcnt, 2, dom, 1, parent, pe::SKEW_BAD_FLAGS, -1);
  refused("flags high bit", nullptr, -1, nullptr, nullptr, nullptr, 0x80000001u, dom, 1, parent, pe::SKEW_BAD_FLAGS, -1);
  check("no book, no jobs", pe::skew_plan_build(p, 0, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, 1, nullptr, 2, 3, sizes,
                                                parent, 9) == pe::SKEW_OK && p.skew.empty() && p.dry_run && !p.constrained() && p.book.empty() &&
                                p.book_off == Vec({0}) && p.n_keys == 3);
  printf("%ld plans, %ld refusals, %d failures\n", plans, refusals, failed);
  return failed ? 1 : 0;
}
