// Placed gangs in the shape the placement calls take and return -- gang v has the groups [group_off[v],
// group_off[v + 1]) with group_count and group_req, and pod_node holds the GLOBAL node id of every pod slot, groups
// in input order (a group of count c owns c slots), -1 = slot skipped: what pe_gang_preempt_domains (its victims)
// and pe_release_gangs / pe_assume_gangs refuse about them, and the walk over a group's slots that merges every run
// of one node into one (node, run length).  Plain C++, no HIP.
#ifndef PE_GANG_SLOTS_H_
#define PE_GANG_SLOTS_H_

#include <stdint.h>

namespace pe {

enum GangSlotsError {
  GANGS_OK = 0,
  GANGS_BAD_COUNT = 1,      // n_gangs outside [0, 2^31 - 1]
  GANGS_NO_OFF = 2,         // group_off NULL (n_gangs > 0)
  GANGS_BAD_OFF = 3,        // group_off does not rise from 0; index = the offset
  GANGS_NO_GROUPS = 4,      // group_count or group_req NULL with groups
  GANGS_BAD_GROUP_COUNT = 5,   // a negative count; index = the group
  GANGS_BAD_REQ = 6,        // a negative request; index = the group
  GANGS_NO_POD_NODE = 7,    // pod_node NULL although some group has pods
  GANGS_BAD_POD_NODE = 8    // a pod_node outside [-1, n_total); index = the pod slot
};

// The checks in the order of the list above; the first offence is reported, *bad_index (if given) receives its
// index (-1 where the error has none).  *slots (if given) receives the number of pod slots of a valid input.
inline GangSlotsError gang_slots_check(int64_t n_gangs, const int32_t* group_off, const int32_t* group_count,
                                       const int64_t* group_req, const int32_t* pod_node, int64_t n_total,
                                       int64_t* slots = nullptr, int64_t* bad_index = nullptr) {
  auto fail = [&](GangSlotsError e, int64_t at) {
    if (bad_index) *bad_index = at;
    return e;
  };
  if (n_gangs < 0 || n_gangs > (int64_t)INT32_MAX) return fail(GANGS_BAD_COUNT, -1);
  const int64_t V = n_gangs;
  int64_t VG = 0;
  if (V > 0) {
    if (!group_off) return fail(GANGS_NO_OFF, -1);
    if (group_off[0] != 0) return fail(GANGS_BAD_OFF, 0);
    for (int64_t v = 0; v < V; ++v)
      if (group_off[v + 1] < group_off[v]) return fail(GANGS_BAD_OFF, v + 1);
    VG = group_off[V];
  }
  int64_t n = 0;
  if (VG > 0) {
    if (!group_count || !group_req) return fail(GANGS_NO_GROUPS, -1);
    for (int64_t g = 0; g < VG; ++g) {
      if (group_count[g] < 0) return fail(GANGS_BAD_GROUP_COUNT, g);
      for (int d = 0; d < 4; ++d)
        if (group_req[g * 4 + d] < 0) return fail(GANGS_BAD_REQ, g);
      n += group_count[g];
    }
  }
  if (n > 0) {
    if (!pod_node) return fail(GANGS_NO_POD_NODE, -1);
    for (int64_t s = 0; s < n; ++s)
      if (pod_node[s] < -1 || pod_node[s] >= n_total) return fail(GANGS_BAD_POD_NODE, s);
  }
  if (slots) *slots = n;
  if (bad_index) *bad_index = -1;
  return GANGS_OK;
}

// The slots [s, s + count) of one group: step(node, run) for every maximal run of one node >= 0, in slot order;
// slots holding -1 end a run and give no step.  s is advanced past the group, or to the end of the run whose step
// returned false (then the walk stops and returns false).
template <class Step>
inline bool gang_group_runs(const int32_t* pod_node, int64_t& s, int32_t count, Step step) {
  const int64_t e = s + count;
  while (s < e) {
    const int32_t node = pod_node[s];
    int64_t run = 1;
    while (s + run < e && pod_node[s + run] == node) ++run;
    s += run;
    if (node >= 0 && !step(node, run)) return false;
  }
  return true;
}

}  // namespace pe

#endif  // PE_GANG_SLOTS_H_
