// The plan of pe_release_gangs / pe_assume_gangs (training-operator_amd/csrc/pe_ledger_plan.h): the touched nodes'
// new residuals, the counted pods, the steps and the refusal's node against a slot-by-slot brute force on random
// inputs with merged runs, -1 slots, removed slots and nodes repeated across gangs; a plan by hand; 100 000 pods on
// one node as one step; products and sums past int64; and every refusal leaving the plan and its scratch untouched.
// Built and run by tests/test_ledger_plan_cpu.py with g++ and the address and undefined-behaviour sanitizers: the
// header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "pe_ledger_plan.h"

using pe::LedgerPlan;

static int failed = 0;
static long plans = 0, slots_checked = 0, nodes_checked = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

struct Mirror {
  std::vector<int64_t> res, res0;   // [n][4]
  int64_t n() const { return (int64_t)res.size() / 4; }
};

struct Gangs {
  std::vector<int32_t> off{0}, cnt, pod;
  std::vector<int64_t> req;
};

static pe::LedgerPlanError build(LedgerPlan& p, pe::LedgerOp op, const Mirror& m, const Gangs& g, int64_t* bad = nullptr,
                                 pe::GangSlotsError* ge = nullptr) {
  return pe::ledger_plan_build(
      p, op, m.n(), (int64_t)g.off.size() - 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(),
      [&m](int32_t n) { return &m.res[(size_t)n * 4]; }, [&m](int32_t n) { return &m.res0[(size_t)n * 4]; }, ge, bad);
}

static bool clean(const LedgerPlan& p) {
  return std::all_of(p.place.begin(), p.place.end(), [](int32_t x) { return x == -1; });
}

static bool same_touched(const std::vector<pe::LedgerUpd>& a, const std::vector<pe::LedgerUpd>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].node != b[i].node || !std::equal(a[i].res, a[i].res + 4, b[i].res)) return false;
  return true;
}

// Slot by slot, no merging: the residuals in 128 bits, the first slot at which the bound is crossed.
struct Brute {
  std::map<int32_t, std::vector<__int128>> res;   // touched node -> residuals
  std::vector<int32_t> order;                     // ... in the order of the first counted slot
  int64_t pods = 0, steps = 0, crossed = -1;
};

static Brute brute(pe::LedgerOp op, const Mirror& m, const Gangs& g) {
  Brute b;
  int64_t s = 0;
  for (size_t v = 0; v + 1 < g.off.size(); ++v)
    for (int32_t gr = g.off[v]; gr < g.off[v + 1]; ++gr) {
      int32_t prev = -1;
      for (int32_t k = 0; k < g.cnt[(size_t)gr]; ++k, ++s) {
        const int32_t node = g.pod[(size_t)s];
        const bool counts = node >= 0 && m.res[(size_t)node * 4] != pe::LEDGER_REMOVED;
        if (counts && node != prev) ++b.steps;
        prev = node;
        if (!counts) continue;
        if (!b.res.count(node)) {
          b.res[node] = {m.res[(size_t)node * 4], m.res[(size_t)node * 4 + 1], m.res[(size_t)node * 4 + 2],
                         m.res[(size_t)node * 4 + 3]};
          b.order.push_back(node);
        }
        for (int d = 0; d < 4; ++d) {
          const int64_t q = g.req[(size_t)gr * 4 + d];
          if (q == 0) continue;
          __int128& r = b.res[node][(size_t)d];
          r += op == pe::LEDGER_RELEASE ? (__int128)q : -(__int128)q;
          if (op == pe::LEDGER_RELEASE ? r > (__int128)m.res0[(size_t)node * 4 + d] : r < 0) {
            b.crossed = node;
            return b;
          }
        }
        ++b.pods;
      }
    }
  return b;
}

// Gangs with runs of one node, -1 slots, zero counts, zero requests and nodes repeated across groups and gangs.
static Gangs random_gangs(std::mt19937& rng, int V, int64_t n_total, int64_t max_req) {
  Gangs g;
  for (int v = 0; v < V; ++v) {
    const int groups = (int)(rng() % 4);
    for (int k = 0; k < groups; ++k) {
      const int c = rng() % 5 == 0 ? 0 : 1 + (int)(rng() % 9);
      g.cnt.push_back(c);
      for (int d = 0; d < 4; ++d) g.req.push_back(rng() % 3 == 0 ? 0 : (int64_t)(rng() % (uint64_t)max_req));
      int32_t node = (int32_t)(rng() % (uint64_t)n_total);
      for (int s = 0; s < c; ++s) {
        if (rng() % 3 == 0) node = rng() % 4 == 0 ? -1 : (int32_t)(rng() % (uint64_t)n_total);   // else: the run goes on
        g.pod.push_back(node);
      }
    }
    g.off.push_back((int32_t)g.cnt.size());
  }
  return g;
}

// What the gangs hold per node and dimension, removed slots included (they are skipped by both sides).
static std::vector<int64_t> totals(const Gangs& g, int64_t n_total) {
  std::vector<int64_t> t((size_t)n_total * 4, 0);
  int64_t s = 0;
  for (size_t gr = 0; gr < g.cnt.size(); ++gr)
    for (int32_t k = 0; k < g.cnt[gr]; ++k, ++s)
      if (g.pod[(size_t)s] >= 0)
        for (int d = 0; d < 4; ++d) t[(size_t)g.pod[(size_t)s] * 4 + d] += g.req[gr * 4 + d];
  return t;
}

static void compare(const char* name, pe::LedgerOp op, const Mirror& m, const Gangs& g, LedgerPlan& plan) {
  const LedgerPlan before = plan;
  int64_t bad = -7;
  const pe::LedgerPlanError e = build(plan, op, m, g, &bad);
  const Brute b = brute(op, m, g);
  ++plans;
  slots_checked += (long)g.pod.size();
  check(name, clean(plan) && (int64_t)plan.place.size() == m.n());
  if (b.crossed >= 0) {
    ++refusals;
    check(name, e == (op == pe::LEDGER_RELEASE ? pe::LEDGER_OVER : pe::LEDGER_UNDER) && bad == b.crossed);
    check(name, same_touched(plan.touched, before.touched) && plan.pods == before.pods && plan.steps == before.steps);
    return;
  }
  check(name, e == pe::LEDGER_OK && bad == -1 && plan.pods == b.pods && plan.steps == b.steps);
  check(name, plan.touched.size() == b.order.size());
  for (size_t i = 0; i < plan.touched.size() && i < b.order.size(); ++i) {
    const pe::LedgerUpd& u = plan.touched[i];
    bool same = u.node == b.order[i];
    for (int d = 0; d < 4 && same; ++d) same = (__int128)u.res[d] == b.res.at((int32_t)u.node)[(size_t)d];
    check(name, same);
    ++nodes_checked;
  }
}

static void test_random() {
  std::mt19937 rng(20261020);
  LedgerPlan plan;   // one plan through all the calls: its scratch map is reused and must come back clean
  for (int it = 0; it < 300; ++it) {
    const int64_t n = 1 + (int64_t)(rng() % 40);
    const Gangs g = random_gangs(rng, 1 + (int)(rng() % 12), n, it % 7 == 0 ? (int64_t)1 << 61 : 100000);
    const std::vector<int64_t> t = totals(g, n);
    Mirror m;
    m.res.resize((size_t)n * 4);
    m.res0.resize((size_t)n * 4);
    // kinds: 0 = the gangs are exactly what was taken; 1 = one unit short somewhere; 2 = anything
    const int kind = it % 3;
    for (int64_t c = 0; c < n * 4; ++c) {
      const int64_t slack = (int64_t)(rng() % 1000);
      if (kind == 2) {
        m.res0[(size_t)c] = (int64_t)(rng() % 400000) - 1000;
        m.res[(size_t)c] = m.res0[(size_t)c] - (int64_t)(rng() % 200000);
      } else if (t[(size_t)c] == 0) {   // a cell the gangs do not move may be negative
        m.res0[(size_t)c] = slack - 500;
        m.res[(size_t)c] = m.res0[(size_t)c] - (int64_t)(rng() % 3);
      } else {
        m.res0[(size_t)c] = t[(size_t)c] + slack;   // the gangs fit an empty node ...
        m.res[(size_t)c] = slack;                   // ... and are what is missing from it now
      }
    }
    for (int64_t node = 0; node < n; ++node)
      if (rng() % 9 == 0) m.res[(size_t)node * 4] = pe::LEDGER_REMOVED;
    if (kind == 1 && !g.pod.empty()) {   // one unit too many on one node in one dimension, for both operations
      const int64_t c = (int64_t)(rng() % (uint64_t)(n * 4));
      if (t[(size_t)c] > 0 && m.res[(size_t)(c / 4) * 4] != pe::LEDGER_REMOVED) m.res0[(size_t)c] -= 1;
    }
    compare("random release", pe::LEDGER_RELEASE, m, g, plan);
    Mirror taken = m;   // the state after the release: the assume of the same gangs leads back
    if (kind == 0) {
      for (const pe::LedgerUpd& u : plan.touched)
        for (int d = 0; d < 4; ++d) taken.res[(size_t)u.node * 4 + d] = u.res[d];
      compare("random assume back", pe::LEDGER_ASSUME, taken, g, plan);
      bool back = true;
      for (const pe::LedgerUpd& u : plan.touched)
        for (int d = 0; d < 4; ++d) back &= u.res[d] == m.res[(size_t)u.node * 4 + d];
      check("release then assume is the identity", back);
    } else {
      if (kind == 1)
        for (int64_t c = 0; c < n * 4; ++c)
          if (m.res[(size_t)c] != pe::LEDGER_REMOVED) taken.res[(size_t)c] = t[(size_t)c] - (c % 5 == 0 ? 1 : 0);
      compare("random assume", pe::LEDGER_ASSUME, taken, g, plan);
    }
  }
  check("the random inputs show both refusals and successes", refusals > 50 && plans - refusals > 150);
}

static void test_by_hand() {
  // nodes 0..3; node 2 is a removed slot.  Gang 0: group 0 = 3 pods {10, 1, 0, 0} on 1, 1, 3; group 1 = 2 pods
  // {0, 0, 2, 0} on -1, 1.  Gang 1: group 2 = 2 pods {5, 0, 0, 7} on 2, 3.
  Mirror m;
  m.res = {100, 100, 100, 100, 50, 50, 50, -3, pe::LEDGER_REMOVED, 0, 0, 0, 7, -9, 7, 7};
  m.res0 = {100, 100, 100, 100, 70, 52, 54, -3, 0, 0, 0, 0, 30, -8, 7, 14};
  Gangs g;
  g.off = {0, 2, 3};
  g.cnt = {3, 2, 2};
  g.req = {10, 1, 0, 0, 0, 0, 2, 0, 5, 0, 0, 7};
  g.pod = {1, 1, 3, -1, 1, 2, 3};
  LedgerPlan p;
  int64_t bad = 0;
  check("hand release", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OK && bad == -1);
  // steps: (1, 2 pods), (3, 1), (1, 1), (3, 1); the pod on the removed slot and the -1 slot count nothing
  check("hand release pods and steps", p.pods == 5 && p.steps == 4 && p.touched.size() == 2 && clean(p));
  const pe::LedgerUpd w1{1, {70, 52, 52, -3}}, w3{3, {22, -8, 7, 14}};
  check("hand release values", same_touched(p.touched, {w1, w3}));
  // node 3's memory at its snapshot: one unit back is one too many, and node 1, earlier in slot order, passed
  m.res0[3 * 4 + 1] = -9;
  const LedgerPlan before = p;
  check("hand release over", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OVER && bad == 3);
  check("hand release over leaves the plan", same_touched(p.touched, before.touched) && p.pods == 5 && p.steps == 4 && clean(p));
  // assume: node 1 has what is asked (its -3 of storage is not moved); node 3 has 7 cpu against 10 + 5
  check("hand assume under", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_UNDER && bad == 3);
  check("hand assume under leaves the plan", same_touched(p.touched, before.touched) && p.pods == 5 && clean(p));
  m.res[3 * 4 + 0] = 15;
  m.res[3 * 4 + 1] = 1;
  check("hand assume", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_OK && p.pods == 5 && p.steps == 4);
  const pe::LedgerUpd a1{1, {30, 48, 48, -3}}, a3{3, {0, 0, 7, 0}};
  check("hand assume values", same_touched(p.touched, {a1, a3}));
}

static void test_assume_by_hand_second_node() {
  // node 3 of the case above on its own: 7 cpu against 10 + 5 asked -- refused at 3, after node 1 passed
  Mirror m;
  m.res = {50, 50, 50, 50, 7, 5, 7, 7};
  m.res0 = m.res;
  Gangs g;
  g.off = {0, 1};
  g.cnt = {3};
  g.req = {5, 1, 0, 0};
  g.pod = {0, 1, 1};
  LedgerPlan p;
  int64_t bad = 0;
  check("second node under", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_UNDER && bad == 1 && clean(p));
  m.res[1 * 4] = 10;
  check("second node exact", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_OK && p.touched[1].res[0] == 0 &&
                                 p.touched[1].res[1] == 3 && p.pods == 3 && p.steps == 2);
}

static void test_one_step() {
  // 100 000 pods of one group on one node are one step, whatever the request
  Mirror m;
  m.res = {0, 5, 0, 0, 1, 1, 1, 1};
  m.res0 = {300000, 5, 0, 100000, 1, 1, 1, 1};
  Gangs g;
  g.off = {0, 2};
  g.cnt = {100000, 100000};
  g.req = {3, 0, 0, 1, 0, 0, 0, 0};
  g.pod.assign(200000, 0);
  LedgerPlan p;
  check("100000 pods", build(p, pe::LEDGER_RELEASE, m, g) == pe::LEDGER_OK && p.steps == 2 && p.pods == 200000);
  check("100000 pods values", p.touched.size() == 1 && p.touched[0].res[0] == 300000 && p.touched[0].res[1] == 5 &&
                                  p.touched[0].res[3] == 100000);
  m.res0[0] = 299999;
  int64_t bad = -1;
  check("100000 pods, one unit short", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OVER && bad == 0);
}

static void test_wide() {
  // k x req past int64: 4 x 2^62 = 2^64 wraps to 0 in 64 bits and would pass every bound
  Mirror m;
  m.res = {0, 0, 0, 0};
  m.res0 = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
  Gangs g;
  g.off = {0, 1};
  g.cnt = {4};
  g.req = {(int64_t)1 << 62, 0, 0, 0};
  g.pod = {0, 0, 0, 0};
  LedgerPlan p;
  int64_t bad = -1;
  check("product past int64, release", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OVER && bad == 0);
  m.res = m.res0;
  check("product past int64, assume", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_UNDER && bad == 0);
  // the same as a sum of separate steps: 2^62 four times with another node in between
  m.res = {0, 0, 0, 0, 0, 0, 0, 0};
  m.res0 = {INT64_MAX, 0, 0, 0, 0, 0, 0, 0};
  g.cnt = {8};
  g.req = {(int64_t)1 << 62, 0, 0, 0};
  g.pod = {0, -1, 0, -1, 0, -1, 0, -1};
  check("sum past int64, release", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OVER && bad == 0);
  // ... and what just fits does: 2^62 + 2^62 - 1 + ... up to INT64_MAX exactly
  g.cnt = {1, 1};
  g.off = {0, 2};
  g.req = {INT64_MAX - 5, 0, 0, 0, 5, 0, 0, 0};
  g.pod = {0, 0};
  check("INT64_MAX exactly", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OK && p.touched[0].res[0] == INT64_MAX);
  m.res[0] = INT64_MAX;
  check("INT64_MAX back", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_OK && p.touched[0].res[0] == 0);
  m.res[0] = INT64_MAX - 1;
  check("INT64_MAX - 1 is one short", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_UNDER && bad == 0);
}

static void test_refusals() {
  Mirror m;
  m.res = {10, 10, 10, 10, 10, 10, 10, 10};
  m.res0 = {20, 20, 20, 20, 20, 20, 20, 20};
  Gangs good;
  good.off = {0, 1};
  good.cnt = {2};
  good.req = {1, 1, 1, 1};
  good.pod = {0, 1};
  LedgerPlan p;
  check("refusals: a good plan first", build(p, pe::LEDGER_RELEASE, m, good) == pe::LEDGER_OK && p.pods == 2);
  const LedgerPlan before = p;
  auto refused = [&](const char* name, const Gangs& g, int64_t n_gangs, const int32_t* off, const int32_t* cnt,
                     const int64_t* req, const int32_t* pod, pe::GangSlotsError want, int64_t want_at) {
    for (pe::LedgerOp op : {pe::LEDGER_RELEASE, pe::LEDGER_ASSUME}) {
      pe::GangSlotsError ge = pe::GANGS_OK;
      int64_t bad = -5;
      const pe::LedgerPlanError e = pe::ledger_plan_build(
          p, op, m.n(), n_gangs, off, cnt, req, pod, [&m](int32_t n) { return &m.res[(size_t)n * 4]; },
          [&m](int32_t n) { return &m.res0[(size_t)n * 4]; }, &ge, &bad);
      check(name, e == pe::LEDGER_BAD_GANGS && ge == want && bad == want_at);
      check(name, same_touched(p.touched, before.touched) && p.pods == before.pods && p.steps == before.steps && clean(p));
    }
    (void)g;
  };
  Gangs g = good;
  refused("n_gangs < 0", g, -1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_COUNT, -1);
  refused("n_gangs above 2^31 - 1", g, (int64_t)INT32_MAX + 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(),
          pe::GANGS_BAD_COUNT, -1);
  refused("no offsets", g, 1, nullptr, g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_NO_OFF, -1);
  g.off = {1, 1};
  refused("offsets not from 0", g, 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_OFF, 0);
  g.off = {0, 1, 0};
  refused("offsets falling", g, 2, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_OFF, 2);
  g = good;
  refused("no counts", g, 1, g.off.data(), nullptr, g.req.data(), g.pod.data(), pe::GANGS_NO_GROUPS, -1);
  refused("no requests", g, 1, g.off.data(), g.cnt.data(), nullptr, g.pod.data(), pe::GANGS_NO_GROUPS, -1);
  g.cnt = {-1};
  refused("negative count", g, 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_GROUP_COUNT, 0);
  g = good;
  g.req = {1, 1, -1, 1};
  refused("negative request", g, 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_REQ, 0);
  g = good;
  refused("no pod nodes", g, 1, g.off.data(), g.cnt.data(), g.req.data(), nullptr, pe::GANGS_NO_POD_NODE, -1);
  g.pod = {0, 2};
  refused("pod node past the inventory", g, 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_POD_NODE, 1);
  g.pod = {-2, 1};
  refused("pod node below -1", g, 1, g.off.data(), g.cnt.data(), g.req.data(), g.pod.data(), pe::GANGS_BAD_POD_NODE, 0);
  // no gangs, and gangs without pods: fine, nothing touched
  check("no gangs", pe::ledger_plan_build(p, pe::LEDGER_RELEASE, m.n(), 0, nullptr, nullptr, nullptr, nullptr,
                                          [&m](int32_t n) { return &m.res[(size_t)n * 4]; },
                                          [&m](int32_t n) { return &m.res0[(size_t)n * 4]; }) == pe::LEDGER_OK &&
                        p.touched.empty() && p.pods == 0 && p.steps == 0);
  g = good;
  g.cnt = {0};
  check("no pods, no pod nodes", pe::ledger_plan_build(p, pe::LEDGER_ASSUME, m.n(), 1, g.off.data(), g.cnt.data(),
                                                       g.req.data(), nullptr,
                                                       [&m](int32_t n) { return &m.res[(size_t)n * 4]; },
                                                       [&m](int32_t n) { return &m.res0[(size_t)n * 4]; }) == pe::LEDGER_OK &&
                                     p.touched.empty() && p.pods == 0);
  // the excess visible only as a total over two gangs; nothing of the first gang stays behind
  g = good;
  g.off = {0, 1, 2};
  g.cnt = {2, 2};
  g.req = {5, 0, 0, 0, 6, 0, 0, 0};
  g.pod = {0, 1, 1, 1};
  int64_t bad = -1;
  check("two gangs over", build(p, pe::LEDGER_RELEASE, m, g, &bad) == pe::LEDGER_OVER && bad == 1 && clean(p));
  check("two gangs under", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_UNDER && bad == 1 && clean(p));
  g.req = {5, 0, 0, 0, 2, 0, 0, 0};
  check("two gangs fit", build(p, pe::LEDGER_ASSUME, m, g, &bad) == pe::LEDGER_OK && p.touched[1].res[0] == 1);
}

int main() {
  test_random();
  test_by_hand();
  test_assume_by_hand_second_node();
  test_one_step();
  test_wide();
  test_refusals();
  printf("%ld plans, %ld slots, %ld nodes checked, %ld refusals, %d failures\n", plans, slots_checked, nodes_checked, refusals,
         failed);
  return failed ? 1 : 0;
}
