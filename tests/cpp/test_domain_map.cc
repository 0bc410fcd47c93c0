// What the domain calls' plans share (training-operator_amd/csrc/pe_domain_map.h): the leaf -> level map, the
// numbering of the active domains, the deal of items to their domains and the pod offsets, against a brute force.
// Built and run by tests/test_domain_map_cpu.py with g++ and the address and undefined-behaviour sanitizers: the
// header needs neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_domain_map.h"

static int failed = 0;
static long maps = 0, leaves_checked = 0, items_checked = 0;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

// The maps and the deal of (hierarchy, level, items) against a scan per leaf, per domain and per item.  order:
// a permutation of the items, or empty for ascending index.
static void verify(const char* name, const std::vector<int32_t>& sizes, const std::vector<int32_t>& parent, int32_t level,
                   const std::vector<int32_t>& dom, const std::vector<int32_t>& order) {
  pe::TreePlan tree;
  const pe::TreePlanError te =
      pe::tree_plan_build(tree, (int32_t)sizes.size(), sizes.data(), parent.empty() ? nullptr : parent.data());
  check(name, te == pe::TREE_OK);
  if (te != pe::TREE_OK) return;
  ++maps;
  const int64_t n = (int64_t)dom.size();
  std::vector<int32_t> leaf_dom(3, 7), act_of(5, 9), active(2, 1);   // whatever they held goes
  pe::domain_map_build(tree, parent.empty() ? nullptr : parent.data(), level, n, dom.empty() ? nullptr : dom.data(),
                       leaf_dom, act_of, active);
  // leaf -> level, one step at a time
  check(name, (int32_t)leaf_dom.size() == sizes[0]);
  for (int32_t k = 0; k < sizes[0] && k < (int32_t)leaf_dom.size(); ++k) {
    int32_t d = k, off = 0;
    for (int l = 0; l < level && d >= 0; ++l) {
      d = parent[(size_t)(off + d)];
      off += sizes[(size_t)l];
    }
    check(name, leaf_dom[(size_t)k] == d);
    ++leaves_checked;
  }
  // active domains: ascending, exactly those some item names
  const int32_t n_dom = sizes[(size_t)level];
  check(name, (int32_t)act_of.size() == n_dom);
  std::vector<int32_t> want_active;
  for (int32_t d = 0; d < n_dom; ++d)
    if (std::find(dom.begin(), dom.end(), d) != dom.end()) want_active.push_back(d);
  check(name, active == want_active);
  if ((int32_t)act_of.size() != n_dom || active != want_active) return;
  for (int32_t d = 0; d < n_dom; ++d) {
    const auto it = std::find(want_active.begin(), want_active.end(), d);
    check(name, act_of[(size_t)d] == (it == want_active.end() ? -1 : (int32_t)(it - want_active.begin())));
  }
  // the deal: domain a's items, in the given order
  std::vector<int32_t> start(4, 3), items(6, 2);
  pe::csr_deal(active.size(), n, [&](int64_t i) { return act_of[(size_t)dom[(size_t)i]]; },
               order.empty() ? nullptr : order.data(), start, items);
  check(name, start.size() == active.size() + 1 && (int64_t)items.size() == n && start[0] == 0 && start.back() == (int32_t)n);
  if (start.size() != active.size() + 1 || (int64_t)items.size() != n) return;
  for (size_t a = 0; a < active.size(); ++a) {
    std::vector<int32_t> want;
    for (int64_t i = 0; i < n; ++i) {
      const int32_t x = order.empty() ? (int32_t)i : order[(size_t)i];
      if (dom[(size_t)x] == active[a]) want.push_back(x);
    }
    check(name, start[a] >= 0 && start[a + 1] >= start[a] && start[a + 1] <= (int32_t)n &&
                    (size_t)(start[a + 1] - start[a]) == want.size() && !want.empty() &&
                    std::equal(want.begin(), want.end(), items.begin() + start[a]));
    items_checked += (long)want.size();
  }
}

// n items over [0, n_dom), most of them in a few domains; a shuffled order for every second call
static void with_items(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes,
                       const std::vector<int32_t>& parent, int32_t level, int n) {
  const int32_t n_dom = sizes[(size_t)level];
  std::vector<int32_t> dom, order;
  for (int i = 0; i < n; ++i)
    dom.push_back((int32_t)(rng() % 3 == 0 ? rng() % (uint32_t)n_dom : rng() % (uint32_t)std::min<int32_t>(n_dom, 3)));
  if (rng() % 2) {
    for (int i = 0; i < n; ++i) order.push_back(i);
    std::shuffle(order.begin(), order.end(), rng);
  }
  verify(name, sizes, parent, level, dom, order);
}

static std::vector<int32_t> concat(std::initializer_list<std::vector<int32_t>> parts) {
  std::vector<int32_t> out;
  for (const auto& v : parts) out.insert(out.end(), v.begin(), v.end());
  return out;
}

// every level, the leaf level and the top level among them, with items and with none
static void all_levels(const char* name, std::mt19937& rng, const std::vector<int32_t>& sizes,
                       const std::vector<int32_t>& parent) {
  for (int32_t level = 0; level < (int32_t)sizes.size(); ++level) {
    with_items(name, rng, sizes, parent, level, 60);
    with_items(name, rng, sizes, parent, level, 0);
  }
}

int main() {
  std::mt19937 rng(29);
  // ---- the hierarchies the engine's tests use (tests/tree_capacity.py at 2500 nodes)
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
    std::vector<int32_t> p0, p1;   // leaves and racks with parent -1: their leaves map to no domain above
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
  // ---- by hand: the deal keeps the given order inside a domain, and ascending index without one
  {
    const std::vector<int32_t> dom = {3, 0, 3, 0, 0, 3};
    verify("ascending", {4}, {}, 0, dom, {});
    verify("given order", {4}, {}, 0, dom, {5, 4, 3, 2, 1, 0});
    pe::TreePlan tree;
    const int32_t sizes[1] = {4};
    check("tree", pe::tree_plan_build(tree, 1, sizes, nullptr) == pe::TREE_OK);
    std::vector<int32_t> leaf_dom, act_of, active, start, items;
    pe::domain_map_build(tree, nullptr, 0, 6, dom.data(), leaf_dom, act_of, active);
    const int32_t order[6] = {5, 4, 3, 2, 1, 0};
    pe::csr_deal(active.size(), 6, [&](int64_t i) { return act_of[(size_t)dom[(size_t)i]]; }, order, start, items);
    check("by hand", leaf_dom == std::vector<int32_t>({0, 1, 2, 3}) && act_of == std::vector<int32_t>({0, -1, -1, 1}) &&
                         active == std::vector<int32_t>({0, 3}) && start == std::vector<int32_t>({0, 3, 6}) &&
                         items == std::vector<int32_t>({4, 3, 1, 5, 2, 0}));
    const int32_t count[4] = {2, 0, 5, 1};
    check("pod offsets", pe::pod_offsets(4, count) == std::vector<int64_t>({0, 2, 2, 7, 8}) &&
                             pe::pod_offsets(0, nullptr) == std::vector<int64_t>({0}));
  }
  // ---- random maps: 1 .. 4 levels, a fifth of the parents -1, a random level, 0 .. 80 items
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 4);
    std::vector<int32_t> sizes, par;
    for (int l = 0; l < L; ++l) sizes.push_back(1 + (int32_t)(rng() % (it % 7 == 0 ? 700 : 40)));
    for (int l = 0; l + 1 < L; ++l)
      for (int32_t k = 0; k < sizes[(size_t)l]; ++k)
        par.push_back(rng() % 5 == 0 ? -1 : (int32_t)(rng() % (uint32_t)sizes[(size_t)l + 1]));
    with_items("random", rng, sizes, par, (int32_t)(rng() % (uint32_t)L), it % 10 == 0 ? 0 : (int)(rng() % 81));
  }
  printf("%ld maps, %ld leaves, %ld items checked, %d failures\n", maps, leaves_checked, items_checked, failed);
  return failed ? 1 : 0;
}
