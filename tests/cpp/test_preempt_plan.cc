// The plan of pe_gang_preempt_domains (training-operator_amd/csrc/pe_preempt_plan.h): the release records, the
// victim -> record CSR, the pairs' lists in plan order and the per-node sums against a brute force on the named
// hierarchies and random inputs, merged runs and -1 slots, a plan by hand, the smaller units, and every refusal
// leaving the plan untouched.  Built and run by tests/test_preempt_plan_cpu.py with g++ and the address and
// undefined-behaviour sanitizers: the header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

#include "pe_preempt_plan.h"

using pe::PreemptPlan;

static int failed = 0;
static long plans = 0, records_checked = 0, lists_checked = 0, sums_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_recs(const std::vector<pe::PreRec>& a, const std::vector<pe::PreRec>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].node != b[i].node || a[i].sat != b[i].sat || !std::equal(a[i].q, a[i].q + 4, b[i].q)) return false;
  return true;
}

static bool same_plan(const PreemptPlan& a, const PreemptPlan& b) {
  if (a.fit.units.size() != b.fit.units.size()) return false;
  for (size_t i = 0; i < a.fit.units.size(); ++i)
    if (a.fit.units[i].act != b.fit.units[i].act || a.fit.units[i].p0 != b.fit.units[i].p0 || a.fit.units[i].p1 != b.fit.units[i].p1)
      return false;
  return a.fit.level == b.fit.level && a.fit.leaf_dom == b.fit.leaf_dom && a.fit.act_of == b.fit.act_of &&
         a.fit.active == b.fit.active && a.fit.pair_start == b.fit.pair_start && a.fit.pairs == b.fit.pairs &&
         a.fit.unit_start == b.fit.unit_start && a.n_victims == b.n_victims && a.rec_start == b.rec_start &&
         same_recs(a.recs, b.recs) && a.list_start == b.list_start && a.list == b.list && a.sum_node == b.sum_node &&
         a.sum_q == b.sum_q;
}

struct Input {
  std::vector<int32_t> sizes, parent;
  int32_t level = 0, J = 1;
  int64_t n_total = 0;
  std::vector<int32_t> voff{0}, vcnt, vpod;
  std::vector<int64_t> vreq;
  std::vector<int32_t> pj, pd, pvo{0}, pv;
};

static pe::PreemptPlanError build(PreemptPlan& p, const Input& in, pe::FitPlanError* fe = nullptr, pe::TreePlanError* te = nullptr,
                                  int64_t* bad = nullptr) {
  return pe::preempt_plan_build(p, in.J, in.n_total, (int64_t)in.voff.size() - 1, in.voff.data(), in.vcnt.data(), in.vreq.data(),
                                in.vpod.data(), (int64_t)in.pj.size(), in.pj.data(), in.pd.data(), in.pvo.data(), in.pv.data(),
                                in.level, (int32_t)in.sizes.size(), in.sizes.data(), in.parent.empty() ? nullptr : in.parent.data(),
                                fe, te, bad);
}

// Victims with runs of one node, -1 slots, zero counts and zero requests; pairs with lists of distinct victims.
static void random_input(std::mt19937& rng, Input& in, int V, int P, int64_t n_total, int max_list) {
  in.n_total = n_total;
  for (int v = 0; v < V; ++v) {
    const int groups = (int)(rng() % 4);
    for (int g = 0; g < groups; ++g) {
      const int c = rng() % 5 == 0 ? 0 : 1 + (int)(rng() % 9);
      in.vcnt.push_back(c);
      for (int d = 0; d < 4; ++d) in.vreq.push_back(rng() % 4 == 0 ? 0 : (int64_t)(rng() % 100000));
      int32_t node = (int32_t)(rng() % (uint64_t)n_total);
      for (int s = 0; s < c; ++s) {
        if (rng() % 3 == 0) node = rng() % 4 == 0 ? -1 : (int32_t)(rng() % (uint64_t)n_total);   // else: the run goes on
        in.vpod.push_back(node);
      }
    }
    in.voff.push_back((int32_t)in.vcnt.size());
  }
  const int32_t n_dom = in.sizes[(size_t)in.level];
  for (int p = 0; p < P; ++p) {
    in.pj.push_back((int32_t)(rng() % (uint32_t)in.J));
    in.pd.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
    std::vector<int32_t> all((size_t)V);
    for (int v = 0; v < V; ++v) all[(size_t)v] = v;
    std::shuffle(all.begin(), all.end(), rng);
    const int K = std::min<int>(V, (int)(rng() % (uint32_t)(max_list + 1)));
    in.pv.insert(in.pv.end(), all.begin(), all.begin() + K);
    in.pvo.push_back((int32_t)in.pv.size());
  }
}

// The plan against a slot-by-slot brute force.
static void verify(const char* name, const Input& in) {
  PreemptPlan p;
  int64_t bad = 7;
  pe::FitPlanError fe = pe::FIT_BAD_LEVEL;
  pe::TreePlanError te = pe::TREE_BAD_LEVELS;
  const pe::PreemptPlanError e = build(p, in, &fe, &te, &bad);
  check(name, e == pe::PRE_OK && fe == pe::FIT_OK && te == pe::TREE_OK && bad == -1);
  if (e != pe::PRE_OK) return;
  ++plans;
  const int64_t V = (int64_t)in.voff.size() - 1, P = (int64_t)in.pj.size();
  // the fit plan underneath, with the smaller units
  pe::FitPlan f;
  check(name, pe::fit_plan_build(f, in.J, P, in.pj.data(), in.pd.data(), in.level, (int32_t)in.sizes.size(), in.sizes.data(),
                                 in.parent.empty() ? nullptr : in.parent.data(), nullptr, nullptr, pe::PRE_UNIT_PAIRS) == pe::FIT_OK);
  check(name, f.pairs == p.fit.pairs && f.active == p.fit.active && f.unit_start == p.fit.unit_start && f.leaf_dom == p.fit.leaf_dom);
  for (const pe::FitUnit& u : p.fit.units) check(name, u.p1 > u.p0 && u.p1 - u.p0 <= pe::PRE_UNIT_PAIRS);
  // per victim: its records give back, node by node, exactly what its slots hold; no record for -1; within a
  // group no two consecutive records of one node (the run was merged)
  check(name, p.n_victims == V && (int64_t)p.rec_start.size() == V + 1 && p.rec_start[0] == 0 &&
                  p.rec_start.back() == (int32_t)p.recs.size());
  std::map<int32_t, std::vector<uint64_t>> total;   // node -> sums over the whole call
  int64_t slot = 0;
  for (int64_t v = 0; v < V; ++v) {
    std::map<int32_t, std::vector<uint64_t>> want, got;
    int64_t runs = 0;
    for (int32_t g = in.voff[(size_t)v]; g < in.voff[(size_t)v + 1]; ++g) {
      int32_t prev = -2;
      for (int32_t s = 0; s < in.vcnt[(size_t)g]; ++s, ++slot) {
        const int32_t node = in.vpod[(size_t)slot];
        if (node != prev && node >= 0) ++runs;
        prev = node;
        if (node < 0) continue;
        for (auto* m : {&want, &total}) {
          auto& q = (*m)[node];
          q.resize(4, 0);
          for (int d = 0; d < 4; ++d) q[(size_t)d] += (uint64_t)in.vreq[(size_t)g * 4 + (size_t)d];
        }
      }
    }
    check(name, p.rec_start[(size_t)v] <= p.rec_start[(size_t)v + 1] && p.rec_start[(size_t)v + 1] - p.rec_start[(size_t)v] == runs);
    for (int32_t r = p.rec_start[(size_t)v]; r < p.rec_start[(size_t)v + 1]; ++r) {
      const pe::PreRec& rec = p.recs[(size_t)r];
      check(name, rec.node >= 0 && rec.node < in.n_total && rec.sat == 0);
      auto& q = got[rec.node];
      q.resize(4, 0);
      for (int d = 0; d < 4; ++d) q[(size_t)d] += (uint64_t)rec.q[d];
      ++records_checked;
    }
    check(name, want == got);
  }
  // the per-node sums: ascending, one entry per node named, the whole call's total
  check(name, p.sum_node.size() == total.size() && p.sum_q.size() == 4 * total.size() &&
                  std::is_sorted(p.sum_node.begin(), p.sum_node.end()));
  size_t k = 0;
  for (const auto& kv : total) {
    if (k >= p.sum_node.size()) break;
    check(name, p.sum_node[k] == kv.first && std::equal(kv.second.begin(), kv.second.end(), p.sum_q.begin() + 4 * (long)k));
    ++k;
    ++sums_checked;
  }
  // the lists: place i of the plan's pair list holds the caller's list of pair fit.pairs[i], in its order
  check(name, (int64_t)p.list_start.size() == P + 1 && p.list_start[0] == 0 && p.list_start.back() == (int32_t)p.list.size() &&
                  p.list.size() == in.pv.size());
  for (int64_t i = 0; i < P; ++i) {
    const int32_t q = p.fit.pairs[(size_t)i];
    const int32_t a = in.pvo[(size_t)q], b = in.pvo[(size_t)q + 1], s = p.list_start[(size_t)i];
    check(name, p.list_start[(size_t)i + 1] - s == b - a && std::equal(in.pv.begin() + a, in.pv.begin() + b, p.list.begin() + s));
    ++lists_checked;
  }
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

static void all_levels(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent) {
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level) {
    Input in;
    in.sizes = sizes;
    in.parent = parent;
    in.level = level;
    in.J = 25;
    random_input(rng, in, 90, 200, 2500, level == 0 ? 64 : 12);
    verify(name, in);
  }
}

int main() {
  std::mt19937 rng(23);
  // ---- the hierarchies the engine's tests use (tests/tree_capacity.py at 2500 nodes), every level
  {
    std::vector<int32_t> p0, p1(20, 0);
    for (int k = 0; k < 79; ++k) p0.push_back(k / 4);
    all_levels("racks32", rng, {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1, p2(27, 0);
    for (int k = 0; k < 313; ++k) p0.push_back(k / 4);
    for (int k = 0; k < 79; ++k) p1.push_back(k / 3);
    all_levels("four", rng, {313, 79, 27, 1}, concat({p0, p1, p2}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 314; ++k) p0.push_back((int32_t)(rng() % 32));
    for (int k = 0; k < 32; ++k) p1.push_back((int32_t)(rng() % 2));
    all_levels("permuted", rng, {314, 32, 2}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(k % 3 == 1 ? -1 : k / 4);
    for (int k = 0; k < 20; ++k) p1.push_back(k % 2 == 1 ? -1 : 0);
    all_levels("orphans", rng, {79, 20, 1}, concat({p0, p1}));
  }
  {
    std::vector<int32_t> p0, p1;
    for (int k = 0; k < 79; ++k) p0.push_back(2 * (k / 4));
    for (int k = 0; k < 43; ++k) p1.push_back(k % 4 == 0 ? 0 : 2);
    all_levels("childless", rng, {79, 43, 3}, concat({p0, p1}));
  }
  {
    const int fans[5] = {1, 63, 64, 65, 200};
    std::vector<int32_t> p0;
    for (int q = 0; q < 5; ++q) p0.insert(p0.end(), (size_t)fans[q], q);
    std::shuffle(p0.begin(), p0.end(), rng);
    all_levels("fanin", rng, {393, 5, 1}, concat({p0, std::vector<int32_t>(5, 0)}));
  }
  all_levels("flat", rng, {79}, {});
  // ---- random inputs
  for (int it = 0; it < 300; ++it) {
    Input in;
    const int L = 1 + (int)(rng() % 4);
    for (int l = 0; l < L; ++l) in.sizes.push_back(1 + (int32_t)(rng() % 40));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < in.sizes[(size_t)l]; ++k)
        in.parent.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)in.sizes[(size_t)l + 1]));
    in.level = (int32_t)(rng() % (uint32_t)L);
    in.J = 1 + (int32_t)(rng() % 30);
    random_input(rng, in, (int)(rng() % 80), (int)(rng() % (it % 5 == 0 ? 400 : 60)), 1 + (int64_t)(rng() % 3000), it % 4 == 0 ? 64 : 8);
    verify("random", in);
  }
  // ---- a plan by hand: two victims, runs merged, -1 slots skipped, three pairs over two domains
  {
    Input in;
    in.sizes = {3};
    in.J = 2;
    in.n_total = 10;
    in.voff = {0, 2, 3};
    in.vcnt = {5, 0, 4};
    in.vreq = {1, 2, 3, 4, 9, 9, 9, 9, 10, 0, 0, 5};
    in.vpod = {7, 7, -1, 7, 2, /* group 2 */ 2, 2, 2, -1};
    in.pj = {0, 1, 1};
    in.pd = {2, 0, 2};
    in.pvo = {0, 2, 3, 3};
    in.pv = {1, 0, 0};
    PreemptPlan p;
    check("by hand: built", build(p, in) == pe::PRE_OK);
    check("by hand: records", p.rec_start == std::vector<int32_t>({0, 3, 4}) && p.recs.size() == 4);
    if (p.recs.size() == 4) {
      const int64_t a[4] = {2, 4, 6, 8}, b[4] = {1, 2, 3, 4}, c[4] = {30, 0, 0, 15};
      check("by hand: a run of two", p.recs[0].node == 7 && std::equal(a, a + 4, p.recs[0].q));
      check("by hand: the node again after -1", p.recs[1].node == 7 && std::equal(b, b + 4, p.recs[1].q));
      check("by hand: another node", p.recs[2].node == 2 && std::equal(b, b + 4, p.recs[2].q));
      check("by hand: a run of three before -1", p.recs[3].node == 2 && std::equal(c, c + 4, p.recs[3].q));
    }
    check("by hand: sums", p.sum_node == std::vector<int32_t>({2, 7}) &&
                               p.sum_q == std::vector<uint64_t>({31, 2, 3, 19, 3, 6, 9, 12}));
    // plan order: domain 0 (pair 1) first, then domain 2 (pairs 0 and 2)
    check("by hand: lists", p.fit.pairs == std::vector<int32_t>({1, 0, 2}) && p.list_start == std::vector<int32_t>({0, 1, 3, 3}) &&
                                p.list == std::vector<int32_t>({0, 1, 0}));
    // 100 000 slots of one node are one record; a product past int64 saturates and marks the sums
    in.voff = {0, 1, 2};
    in.vcnt = {100000, 3};
    in.vreq = {0, 1, 0, 0, INT64_MAX / 2, 0, 0, 1};
    in.vpod.assign(100000, 4);
    in.vpod.insert(in.vpod.end(), {5, 5, 5});
    check("long run: built", build(p, in) == pe::PRE_OK && p.recs.size() == 2 && p.rec_start == std::vector<int32_t>({0, 1, 2}));
    if (p.recs.size() == 2) {
      check("long run: one record", p.recs[0].node == 4 && p.recs[0].q[1] == 100000 && p.recs[0].sat == 0);
      check("overflow: saturated", p.recs[1].node == 5 && p.recs[1].q[0] == INT64_MAX && p.recs[1].sat == 1 && p.recs[1].q[3] == 3);
      check("overflow: the sums say so", p.sum_node == std::vector<int32_t>({4, 5}) && p.sum_q[4] == UINT64_MAX && p.sum_q[7] == 3);
    }
    // two records that only together pass int64: the sum holds it exactly (the engine compares it with the residual)
    in.voff = {0, 1, 2};
    in.vcnt = {1, 1};
    in.vreq = {INT64_MAX, 0, 0, 0, INT64_MAX, 0, 0, 0};
    in.vpod = {6, 6};
    check("sum past int64", build(p, in) == pe::PRE_OK && p.sum_q[0] == 2 * (uint64_t)INT64_MAX && p.recs[0].sat == 0);
    // no victims, no pairs
    Input none;
    none.sizes = {3};
    none.n_total = 10;
    check("empty", build(p, none) == pe::PRE_OK && p.recs.empty() && p.rec_start == std::vector<int32_t>({0}) &&
                       p.list_start == std::vector<int32_t>({0}) && p.sum_node.empty());
    check("empty: NULL arrays", pe::preempt_plan_build(p, 0, 10, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                                       nullptr, 0, 1, none.sizes.data(), nullptr) == pe::PRE_OK);
  }
  // ---- refusals: the plan stays as it was
  {
    Input good;
    good.sizes = {4, 2, 1};
    good.parent = {0, 1, -1, 1, 0, 0};
    good.level = 1;
    good.J = 2;
    good.n_total = 300;
    good.voff = {0, 1, 3};
    good.vcnt = {2, 1, 2};
    good.vreq = {1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3};
    good.vpod = {5, 6, 7, -1, 299};
    good.pj = {1, 0, 1};
    good.pd = {1, 0, 1};
    good.pvo = {0, 2, 2, 3};
    good.pv = {1, 0, 1};
    PreemptPlan p;
    check("a plan to keep", build(p, good) == pe::PRE_OK);
    const PreemptPlan before = p;
    auto refused = [&](const char* name, const Input& in, pe::PreemptPlanError want, int64_t want_index,
                       pe::FitPlanError want_fit = pe::FIT_OK) {
      int64_t bad = 99;
      pe::FitPlanError fe = pe::FIT_OK;
      check(name, build(p, in, &fe, nullptr, &bad) == want && fe == want_fit && bad == want_index && same_plan(p, before));
      check(name, build(p, in) == want && same_plan(p, before));   // nothing asked for
    };
    auto with = [&](auto change) {
      Input in = good;
      change(in);
      return in;
    };
    refused("the pairs", with([](Input& in) { in.pj[1] = 2; }), pe::PRE_BAD_FIT, 1, pe::FIT_BAD_JOB);
    refused("the level", with([](Input& in) { in.level = 3; }), pe::PRE_BAD_FIT, -1, pe::FIT_BAD_LEVEL);
    refused("the map", with([](Input& in) { in.parent[2] = 2; }), pe::PRE_BAD_FIT, 2, pe::FIT_BAD_TREE);
    refused("offsets from 1", with([](Input& in) { in.voff[0] = 1; }), pe::PRE_BAD_VIC_OFF, 0);
    refused("offsets falling", with([](Input& in) { in.voff = {0, 3, 2}; }), pe::PRE_BAD_VIC_OFF, 2);
    refused("a negative count", with([](Input& in) { in.vcnt[2] = -2; }), pe::PRE_BAD_VIC_COUNT, 2);
    refused("a negative request", with([](Input& in) { in.vreq[6] = -1; }), pe::PRE_BAD_VIC_REQ, 1);
    refused("a node = n_total", with([](Input& in) { in.vpod[4] = 300; }), pe::PRE_BAD_POD_NODE, 4);
    refused("a node below -1", with([](Input& in) { in.vpod[1] = -2; }), pe::PRE_BAD_POD_NODE, 1);
    refused("list offsets from 1", with([](Input& in) { in.pvo[0] = 1; }), pe::PRE_BAD_LIST_OFF, 0);
    refused("list offsets falling", with([](Input& in) { in.pvo = {0, 2, 1, 3}; }), pe::PRE_BAD_LIST_OFF, 2);
    refused("a victim = n_victims", with([](Input& in) { in.pv[2] = 2; }), pe::PRE_BAD_LIST_VICTIM, 2);
    refused("a negative victim", with([](Input& in) { in.pv[0] = -1; }), pe::PRE_BAD_LIST_VICTIM, 0);
    refused("a victim twice", with([](Input& in) { in.pv[1] = 1; }), pe::PRE_DUP_VICTIM, 1);
    refused("a list of 65", with([](Input& in) {
              in.pvo = {0, 2, 67, 68};
              in.pv.assign(68, 0);
            }),
            pe::PRE_LONG_LIST, 1);
    {   // 64 distinct victims are a list; the same victim in several pairs is fine
      Input in = good;
      in.voff.assign(66, 0);
      in.vcnt.clear();
      in.vreq.clear();
      in.vpod.clear();
      in.pvo = {0, 64, 128, 129};
      in.pv.clear();
      for (int r = 0; r < 2; ++r)
        for (int v = 0; v < 64; ++v) in.pv.push_back(v);
      in.pv.push_back(64);
      PreemptPlan q;
      check("lists of 64", build(q, in) == pe::PRE_OK && q.list.size() == 129 && q.recs.empty());
    }
    // the NULL arrays, through the raw call
    auto raw = [&](const int32_t* voff, const int32_t* vcnt, const int64_t* vreq, const int32_t* vpod, const int32_t* pvo,
                   const int32_t* pv, int64_t V, pe::PreemptPlanError want, const char* name) {
      int64_t bad = 99;
      const pe::PreemptPlanError e = pe::preempt_plan_build(p, good.J, good.n_total, V, voff, vcnt, vreq, vpod, 3, good.pj.data(),
                                                            good.pd.data(), pvo, pv, 1, 3, good.sizes.data(), good.parent.data(),
                                                            nullptr, nullptr, &bad);
      check(name, e == want && bad == -1 && same_plan(p, before));
    };
    const Input& g = good;
    raw(nullptr, g.vcnt.data(), g.vreq.data(), g.vpod.data(), g.pvo.data(), g.pv.data(), 2, pe::PRE_NO_VIC_OFF, "no offsets");
    raw(g.voff.data(), nullptr, g.vreq.data(), g.vpod.data(), g.pvo.data(), g.pv.data(), 2, pe::PRE_NO_VIC_GROUPS, "no counts");
    raw(g.voff.data(), g.vcnt.data(), nullptr, g.vpod.data(), g.pvo.data(), g.pv.data(), 2, pe::PRE_NO_VIC_GROUPS, "no requests");
    raw(g.voff.data(), g.vcnt.data(), g.vreq.data(), nullptr, g.pvo.data(), g.pv.data(), 2, pe::PRE_NO_POD_NODE, "no pod nodes");
    raw(g.voff.data(), g.vcnt.data(), g.vreq.data(), g.vpod.data(), nullptr, g.pv.data(), 2, pe::PRE_NO_LIST_OFF, "no list offsets");
    raw(g.voff.data(), g.vcnt.data(), g.vreq.data(), g.vpod.data(), g.pvo.data(), nullptr, 2, pe::PRE_NO_LIST, "no lists");
    raw(g.voff.data(), g.vcnt.data(), g.vreq.data(), g.vpod.data(), g.pvo.data(), g.pv.data(), -1, pe::PRE_BAD_VICTIMS, "n_victims < 0");
    raw(g.voff.data(), g.vcnt.data(), g.vreq.data(), g.vpod.data(), g.pvo.data(), g.pv.data(), (int64_t)INT32_MAX + 1,
        pe::PRE_BAD_VICTIMS, "n_victims above int32");
  }
  printf("%ld plans, %ld records, %ld lists, %ld sums checked, %d failures\n", plans, records_checked, lists_checked, sums_checked,
         failed);
  return failed ? 1 : 0;
}
