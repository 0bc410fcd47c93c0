// What the plans of the domain calls share (pe_place_plan.h, pe_fit_plan.h, pe_first_fit_plan.h).  Plain C++, no
// HIP; tests/cpp/test_domain_map.cc checks it against a brute force.  Every input is validated by the caller.
#ifndef PE_DOMAIN_MAP_H_
#define PE_DOMAIN_MAP_H_

#include <numeric>

#include "pe_tree_plan.h"

namespace pe {

//   leaf_dom[size[0]]    the level-`level` domain of leaf domain k, walked up the parent map; -1 = none
//   act_of[size[level]]  the ACTIVE index of a level-`level` domain (active = named by one of dom[n]), -1 = inactive
//   active[A]            the active domains' ids, ascending
inline void domain_map_build(const TreePlan& tree, const int32_t* parent, int32_t level, int64_t n, const int32_t* dom,
                             std::vector<int32_t>& leaf_dom, std::vector<int32_t>& act_of, std::vector<int32_t>& active) {
  leaf_dom.resize((size_t)tree.size[0]);
  std::iota(leaf_dom.begin(), leaf_dom.end(), 0);
  for (int l = 0; l < level; ++l)   // one step up the parent map per level
    for (int32_t& d : leaf_dom)
      if (d >= 0) d = parent[tree.off[l] + d];
  act_of.assign((size_t)tree.size[level], -1);
  active.clear();
  for (int64_t i = 0; i < n; ++i) act_of[(size_t)dom[i]] = 0;
  for (int32_t d = 0; d < tree.size[level]; ++d)
    if (act_of[(size_t)d] == 0) {
      act_of[(size_t)d] = (int32_t)active.size();
      active.push_back(d);
    }
}

// n items dealt to `bins` bins by key(i) (a counting sort): start[bins + 1] and items[n], bin b's items at
// items[start[b] .. start[b + 1]) in the order of order[n], or in ascending index where order is NULL.
template <class Key>
inline void csr_deal(size_t bins, int64_t n, Key key, const int32_t* order, std::vector<int32_t>& start,
                     std::vector<int32_t>& items) {
  start.assign(bins + 1, 0);
  for (int64_t i = 0; i < n; ++i) ++start[(size_t)key(i) + 1];
  for (size_t b = 0; b < bins; ++b) start[b + 1] += start[b];
  std::vector<int32_t> fill(start.begin(), start.end() - 1);
  items.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int32_t x = order ? order[i] : (int32_t)i;
    items[(size_t)fill[(size_t)key(x)]++] = x;
  }
}

// Each of the G groups' first pod slot, groups in input order: [G + 1].
inline std::vector<int64_t> pod_offsets(int64_t G, const int32_t* group_count) {
  std::vector<int64_t> off((size_t)G + 1, 0);
  for (int64_t g = 0; g < G; ++g) off[(size_t)g + 1] = off[(size_t)g] + group_count[g];
  return off;
}

}  // namespace pe

#endif  // PE_DOMAIN_MAP_H_
