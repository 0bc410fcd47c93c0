// The plan of pe_drain_fit_domains (training-operator_amd/csrc/pe_drain_plan.h): every candidate's evicted slots,
// their runs and the synthetic jobs (candidate c = pair c of the fit plan) against a slot-by-slot brute force on 300
// random books with -1 slots, removed candidates, candidates without pods and nodes shared by many gangs; plans by
// hand for candidates with 0 pods, 1 pod and every pod of the call; counts of 2^31 - 1; and every refusal with its
// index, each leaving the plan and its node -> candidate map untouched.  Built and run by
// tests/test_drain_plan_cpu.py with g++ and the address and undefined-behaviour sanitizers: the header needs
// neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "pe_drain_plan.h"

using pe::DrainPlan;

static int failed = 0;
static long plans = 0, slots_checked = 0, runs_checked = 0, refusals = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

struct Input {
  int64_t n_total = 0;
  std::vector<int32_t> off{0}, cnt, pod, cand_node, cand_domain, level_size{1}, parent;
  std::vector<int64_t> req;
  std::set<int32_t> removed;
  int32_t level = 0;
};

struct Errors {
  pe::GangSlotsError ge = pe::GANGS_OK;
  pe::FitPlanError fe = pe::FIT_OK;
  pe::TreePlanError te = pe::TREE_OK;
  int64_t bad = -7;
};

static pe::DrainPlanError build(DrainPlan& p, const Input& in, Errors* e = nullptr) {
  Errors local;
  Errors& r = e ? *e : local;
  return pe::drain_plan_build(
      p, in.n_total, (int64_t)in.off.size() - 1, in.off.data(), in.cnt.data(), in.req.data(), in.pod.data(),
      (int64_t)in.cand_node.size(), in.cand_node.data(), in.cand_domain.data(), in.level, (int32_t)in.level_size.size(),
      in.level_size.data(), in.parent.empty() ? nullptr : in.parent.data(),
      [&in](int32_t n) { return in.removed.count(n) != 0; }, &r.ge, &r.fe, &r.te, &r.bad);
}

static bool clean(const DrainPlan& p) {
  return std::all_of(p.cand_of.begin(), p.cand_of.end(), [](int32_t x) { return x == -1; });
}

static bool same_runs(const std::vector<pe::DrainRun>& a, const std::vector<pe::DrainRun>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i].group != b[i].group || a[i].count != b[i].count || a[i].pod0 != b[i].pod0) return false;
  return true;
}

static bool same_plan(const DrainPlan& a, const DrainPlan& b) {
  return a.slots == b.slots && a.slot_start == b.slot_start && a.slot_list == b.slot_list && a.run_start == b.run_start &&
         same_runs(a.runs, b.runs) && a.fit.pairs == b.fit.pairs && a.fit.pair_start == b.fit.pair_start &&
         a.fit.active == b.fit.active && a.fit.units.size() == b.fit.units.size();
}

// Candidate by candidate, slot by slot.
static void against_brute(const char* name, const DrainPlan& p, const Input& in) {
  const int64_t C = (int64_t)in.cand_node.size();
  std::vector<int32_t> group_of;
  for (size_t g = 0; g < in.cnt.size(); ++g) group_of.insert(group_of.end(), (size_t)in.cnt[g], (int32_t)g);
  bool ok = p.n_cands() == C && p.slots == (int64_t)group_of.size() && clean(p);
  ok = ok && (int64_t)p.run_start.size() == C + 1 && p.slot_start[0] == 0 && p.run_start[0] == 0;
  for (int64_t c = 0; c < C && ok; ++c) {
    std::vector<int32_t> slots;
    if (!in.removed.count(in.cand_node[(size_t)c]))
      for (size_t s = 0; s < group_of.size(); ++s)
        if (in.pod[s] == in.cand_node[(size_t)c]) slots.push_back((int32_t)s);
    const int64_t s0 = p.slot_start[(size_t)c], s1 = p.slot_start[(size_t)c + 1];
    ok = ok && s1 - s0 == (int64_t)slots.size() &&
         std::equal(slots.begin(), slots.end(), p.slot_list.begin() + (ptrdiff_t)s0);
    if (!ok) break;
    // the runs: maximal stretches of one group, back to back from s0
    int64_t at = s0;
    int32_t r = p.run_start[(size_t)c];
    for (size_t i = 0; i < slots.size();) {
      size_t e = i + 1;
      while (e < slots.size() && group_of[(size_t)slots[e]] == group_of[(size_t)slots[i]]) ++e;
      ok = ok && r < p.run_start[(size_t)c + 1] && p.runs[(size_t)r].group == group_of[(size_t)slots[i]] &&
           p.runs[(size_t)r].count == (int32_t)(e - i) && p.runs[(size_t)r].pod0 == at;
      at += (int64_t)(e - i);
      ++r;
      ++runs_checked;
      i = e;
    }
    ok = ok && r == p.run_start[(size_t)c + 1];
    slots_checked += (long)slots.size();
  }
  // the synthetic jobs: every candidate is exactly one pair, in its domain's range of the pair CSR
  std::vector<int> seen((size_t)C, 0);
  for (size_t a = 0; a < p.fit.active.size() && ok; ++a)
    for (int32_t i = p.fit.pair_start[a]; i < p.fit.pair_start[a + 1]; ++i) {
      const int32_t c = p.fit.pairs[(size_t)i];
      ok = ok && c >= 0 && c < C && in.cand_domain[(size_t)c] == p.fit.active[a] && ++seen[(size_t)c] == 1;
      if (i > p.fit.pair_start[a]) ok = ok && p.fit.pairs[(size_t)i - 1] < c;
    }
  ok = ok && std::all_of(seen.begin(), seen.end(), [](int x) { return x == 1; });
  int64_t in_units = 0;
  for (const pe::FitUnit& u : p.fit.units) {
    ok = ok && u.p1 > u.p0 && u.p1 - u.p0 <= pe::FIT_UNIT_PAIRS;
    in_units += u.p1 - u.p0;
  }
  ok = ok && in_units == C;
  check(name, ok);
  ++plans;
}

static Input random_input(std::mt19937& rng, int k) {
  auto rnd = [&rng](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  Input in;
  in.n_total = rnd(1, k % 7 == 0 ? 400 : 40);
  const int n_dom = rnd(1, 9);
  in.level_size = {(int32_t)n_dom};
  if (k % 5 == 0) {   // two levels: the call's level is the upper one
    in.level_size.push_back((int32_t)rnd(1, 3));
    for (int d = 0; d < n_dom; ++d) in.parent.push_back((int32_t)rnd(-1, in.level_size[1] - 1));
    in.level = 1;
  }
  const int V = rnd(0, 12);
  for (int v = 0; v < V; ++v) {
    const int G = rnd(0, 3);
    for (int g = 0; g < G; ++g) {
      const int c = rnd(0, 9);
      in.cnt.push_back(c);
      for (int d = 0; d < 4; ++d) in.req.push_back(rnd(0, 5));
      int32_t node = (int32_t)rnd(0, (int)in.n_total - 1);
      for (int i = 0; i < c; ++i) {   // pods cluster on a few nodes, with -1 slots in between
        if (rnd(0, 2) == 0) node = (int32_t)rnd(-1, (int)std::min<int64_t>(in.n_total - 1, 7));
        in.pod.push_back(node);
      }
    }
    in.off.push_back((int32_t)in.cnt.size());
  }
  std::vector<int32_t> nodes((size_t)in.n_total);
  for (size_t i = 0; i < nodes.size(); ++i) nodes[i] = (int32_t)i;
  std::shuffle(nodes.begin(), nodes.end(), rng);
  const int C = k % 11 == 0 ? (int)in.n_total : rnd(0, (int)std::min<int64_t>(in.n_total, 70));
  for (int c = 0; c < C; ++c) {
    in.cand_node.push_back(nodes[(size_t)c]);
    in.cand_domain.push_back((int32_t)rnd(0, in.level_size[(size_t)in.level] - 1));
    if (rnd(0, 9) == 0) in.removed.insert(nodes[(size_t)c]);
  }
  return in;
}

static void random_books() {
  std::mt19937 rng(20240607);
  DrainPlan p;   // one plan through all of them, as the engine's: the map is reused and re-sized
  for (int k = 0; k < 300; ++k) {
    const Input in = random_input(rng, k);
    char name[64];
    snprintf(name, sizeof name, "random book %d", k);
    check(name, build(p, in) == pe::DRAIN_OK);
    against_brute(name, p, in);
  }
}

static Input small() {
  Input in;
  in.n_total = 6;
  in.level_size = {3};
  // gang 0: group 0 = 3 pods on (2, 4, 2), group 1 = 2 pods on (2, -1); gang 1: group 2 = 1 pod on 2
  in.off = {0, 2, 3};
  in.cnt = {3, 2, 1};
  in.req = {1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3};
  in.pod = {2, 4, 2, 2, -1, 2};
  in.cand_node = {2, 5, 4};
  in.cand_domain = {1, 1, 0};
  return in;
}

static void by_hand() {
  DrainPlan p;
  Input in = small();
  check("by hand: built", build(p, in) == pe::DRAIN_OK);
  against_brute("by hand", p, in);
  // node 2: slots 0, 2 (group 0: one run although slot 1 lies between), 3 (group 1), 5 (group 2); node 5: no pod;
  // node 4: one pod
  check("by hand: slots", p.slot_start == std::vector<int64_t>({0, 4, 4, 5}) &&
                              p.slot_list == std::vector<int32_t>({0, 2, 3, 5, 1}));
  check("by hand: runs", p.run_start == std::vector<int32_t>({0, 3, 3, 4}) &&
                             same_runs(p.runs, {{0, 2, 0}, {1, 1, 2}, {2, 1, 3}, {0, 1, 4}}));
  check("by hand: domains", p.fit.active == std::vector<int32_t>({0, 1}) && p.fit.pairs == std::vector<int32_t>({2, 0, 1}));
  // every pod of the call on one candidate
  std::fill(in.pod.begin(), in.pod.end(), 3);
  in.cand_node = {3};
  in.cand_domain = {2};
  check("all pods: built", build(p, in) == pe::DRAIN_OK);
  against_brute("all pods", p, in);
  check("all pods: one list", p.n_evicted() == 6 && p.n_runs() == 3 && p.runs[2].pod0 == 5);
  // ... and on a removed candidate: nothing is evicted
  in.removed = {3};
  check("removed: built", build(p, in) == pe::DRAIN_OK);
  against_brute("removed", p, in);
  check("removed: nothing", p.n_evicted() == 0 && p.n_runs() == 0 && p.fit.n_units() == 1);
  // no candidates, no gangs
  in = small();
  in.cand_node.clear();
  in.cand_domain.clear();
  check("no candidates", build(p, in) == pe::DRAIN_OK && p.n_cands() == 0 && p.slots == 6 && p.n_evicted() == 0);
  in = small();
  in.off = {0};
  in.cnt.clear();
  in.req.clear();
  in.pod.clear();
  check("no gangs", build(p, in) == pe::DRAIN_OK && p.n_cands() == 3 && p.slots == 0 && p.n_evicted() == 0);
  against_brute("no gangs", p, in);
}

constexpr int64_t AS_GIVEN = INT64_MIN;   // a count taken from the input's arrays

static void refusals_leave_the_plan() {
  DrainPlan p;
  const Input good = small();
  check("refusals: built", build(p, good) == pe::DRAIN_OK);
  const DrainPlan before = p;
  auto refused = [&](const char* name, const Input& in, pe::DrainPlanError want, int64_t want_bad,
                     int64_t n_cands = AS_GIVEN, bool null_nodes = false, int64_t n_gangs = AS_GIVEN) {
    Errors e;
    const int64_t C = n_cands != AS_GIVEN ? n_cands : (int64_t)in.cand_node.size();
    const pe::DrainPlanError got = pe::drain_plan_build(
        p, in.n_total, n_gangs != AS_GIVEN ? n_gangs : (int64_t)in.off.size() - 1, in.off.data(), in.cnt.data(),
        in.req.data(), in.pod.empty() ? nullptr : in.pod.data(), C, null_nodes ? nullptr : in.cand_node.data(),
        in.cand_domain.data(), in.level, (int32_t)in.level_size.size(), in.level_size.data(),
        in.parent.empty() ? nullptr : in.parent.data(), [](int32_t) { return false; }, &e.ge, &e.fe, &e.te, &e.bad);
    check(name, got == want && e.bad == want_bad && same_plan(p, before) && clean(p));
    ++refusals;
    return e;
  };
  Input in = good;
  in.off = {0, 3, 2};
  check("ge", refused("offsets falling", in, pe::DRAIN_BAD_GANGS, 2).ge == pe::GANGS_BAD_OFF);
  in = good;
  in.cnt[1] = -1;
  check("ge", refused("negative count", in, pe::DRAIN_BAD_GANGS, 1).ge == pe::GANGS_BAD_GROUP_COUNT);
  in = good;
  in.req[9] = -3;
  check("ge", refused("negative request", in, pe::DRAIN_BAD_GANGS, 2).ge == pe::GANGS_BAD_REQ);
  in = good;
  in.pod[3] = 6;
  check("ge", refused("pod_node past n_total", in, pe::DRAIN_BAD_GANGS, 3).ge == pe::GANGS_BAD_POD_NODE);
  in.pod[3] = -2;
  check("ge", refused("pod_node below -1", in, pe::DRAIN_BAD_GANGS, 3).ge == pe::GANGS_BAD_POD_NODE);
  in = good;
  check("ge", refused("n_gangs < 0", in, pe::DRAIN_BAD_GANGS, -1, AS_GIVEN, false, -1).ge == pe::GANGS_BAD_COUNT);
  check("ge", refused("n_gangs 2^31", in, pe::DRAIN_BAD_GANGS, -1, AS_GIVEN, false, (int64_t)INT32_MAX + 1).ge ==
                  pe::GANGS_BAD_COUNT);
  // counts of 2^31 - 1: one group of that many pods needs its pod_node; two of them are more slots than a list holds
  in = good;
  in.off = {0, 1};
  in.cnt = {INT32_MAX};
  in.req.resize(4);
  in.pod.clear();
  check("ge", refused("2^31 - 1 pods, no pod_node", in, pe::DRAIN_BAD_GANGS, -1).ge == pe::GANGS_NO_POD_NODE);
  in = good;
  refused("n_cands 2^31 - 1", in, pe::DRAIN_BAD_COUNT, -1, (int64_t)INT32_MAX);
  refused("n_cands < 0", in, pe::DRAIN_BAD_COUNT, -1, -1);
  refused("n_cands 2^31 - 2, no cand_node", in, pe::DRAIN_NO_CANDS, -1, (int64_t)INT32_MAX - 1, true);
  refused("no cand_node", in, pe::DRAIN_NO_CANDS, -1, AS_GIVEN, true);
  in.cand_node[1] = 6;
  refused("cand_node past n_total", in, pe::DRAIN_BAD_NODE, 1);
  in.cand_node[1] = -1;
  refused("cand_node negative", in, pe::DRAIN_BAD_NODE, 1);
  in = good;
  in.cand_node[2] = 2;
  refused("cand_node twice", in, pe::DRAIN_DUP_NODE, 2);
  in = good;
  in.cand_domain[1] = 3;
  check("fe", refused("cand_domain past the level", in, pe::DRAIN_BAD_FIT, 1).fe == pe::FIT_BAD_DOMAIN);
  in.cand_domain[1] = -1;
  check("fe", refused("cand_domain negative", in, pe::DRAIN_BAD_FIT, 1).fe == pe::FIT_BAD_DOMAIN);
  in = good;
  in.level = 1;
  check("fe", refused("level past the levels", in, pe::DRAIN_BAD_FIT, -1).fe == pe::FIT_BAD_LEVEL);
  in.level = -1;
  check("fe", refused("level negative", in, pe::DRAIN_BAD_FIT, -1).fe == pe::FIT_BAD_LEVEL);
  in = good;
  in.level_size = {0};
  {
    const Errors e = refused("level_size 0", in, pe::DRAIN_BAD_FIT, 0);
    check("te", e.fe == pe::FIT_BAD_TREE && e.te == pe::TREE_BAD_SIZE);
  }
  in.level_size = {3, 2};   // two levels without a parent map
  {
    const Errors e = refused("no parent", in, pe::DRAIN_BAD_FIT, -1);
    check("te", e.fe == pe::FIT_BAD_TREE && e.te == pe::TREE_NO_PARENT);
  }
  // the plan still works after all of them
  check("after the refusals", build(p, good) == pe::DRAIN_OK && same_plan(p, before));
  against_brute("after the refusals", p, good);
}

int main() {
  random_books();
  by_hand();
  refusals_leave_the_plan();
  printf("%ld plans, %ld slots, %ld runs checked, %ld refusals, %d failures\n", plans, slots_checked, runs_checked, refusals,
         failed);
  return failed ? 1 : 0;
}
