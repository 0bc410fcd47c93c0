// The host side of pe_gang_slice_tree and the one piece of arithmetic it shares with the kernels of
// pe_slice.hip.  Plain C++, no HIP: the engine includes it on the host, the kernels for slice_units, and
// tests/cpp/test_slice_plan.cc builds it under the sanitizers.
//
// A job asks for count pods in slices of z = slice_size pods, each slice inside one domain of level
// sl = slice_level (SLICE_NODE: inside one node).  The device tables get one ROW per distinct
// (shape, z, sl) -- slots below level m = max(sl, 0), units (whole slices) at and above it -- and the
// selection and the descent run once per distinct PICK (row, units wanted, max_level).  z = 1 with sl <= 0
// asks for what pe_gang_split_tree answers, whichever of the two levels it names: both are the row
// (shape, 1, 0).  Rows and picks are numbered in first-seen order (pe_first_seen.h); the chunk of device
// tables a row lands in follows from its number.
#ifndef PE_SLICE_PLAN_H_
#define PE_SLICE_PLAN_H_

#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PE_SL_HD __host__ __device__ __forceinline__
#elif defined(__HIPCC__)
#define PE_SL_HD __host__ __device__ inline
#else
#define PE_SL_HD inline
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

#include "pe_first_seen.h"
#endif

namespace pe {

constexpr int SLICE_NODE = -1;   // PE_SLICE_NODE

// The unit conversion: the whole slices of z pods (z >= 1) that x slots hold.  A node's capacity (at most
// PE_CAP_MAX) at node level, a domain's slots (below 2^55) at level sl.
PE_SL_HD uint64_t slice_units(uint64_t x, uint32_t z) { return z == 1 ? x : x / z; }

// One row of the device tables.  16 B: the kernels read it through a uniform address.
struct SliceRow {
  uint32_t shape;   // index into the call's distinct (request, need) shapes
  int32_t z;        // >= 1
  int32_t sl;       // SLICE_NODE or a level; never SLICE_NODE with z == 1 (the canonical form)
  int32_t pad_;
};
static_assert(sizeof(SliceRow) == 16, "SliceRow must be 16 B");
PE_SL_HD bool operator==(const SliceRow& a, const SliceRow& b) { return a.shape == b.shape && a.z == b.z && a.sl == b.sl; }

// The row of (shape, z, sl) in its canonical form.
PE_SL_HD SliceRow slice_row(uint32_t shape, int32_t z, int32_t sl) {
  return SliceRow{shape, z, (z == 1 && sl < 0) ? 0 : sl, 0};
}
// The lowest level a row's selection may name, and the level whose list the descent turns from units to pods.
PE_SL_HD int32_t slice_floor(int32_t sl) { return sl < 0 ? 0 : sl; }

#if !defined(__HIP_DEVICE_COMPILE__)
// What the call refuses beyond pe_gang_split_tree's refusals, in the order checked; each check scans the whole
// batch and reports its first offending job.  count[j] >= 1 and max_level[j] in [0, n_levels) hold already.
// slice_size NULL = 1, slice_level NULL = 0, max_level NULL = n_levels - 1 for every job.
enum SliceError { SLICE_OK = 0, SLICE_BAD_SIZE, SLICE_BAD_COUNT, SLICE_BAD_LEVEL, SLICE_BAD_MAX_LEVEL };
inline SliceError slice_validate(int64_t n, const int32_t* count, const int32_t* slice_size, const int32_t* slice_level,
                                 const int32_t* max_level, int32_t n_levels, int64_t* bad) {
  if (slice_size) {
    for (int64_t j = 0; j < n; ++j)
      if (slice_size[j] < 1) return *bad = j, SLICE_BAD_SIZE;
    for (int64_t j = 0; j < n; ++j)
      if (count[j] % slice_size[j] != 0) return *bad = j, SLICE_BAD_COUNT;
  }
  if (slice_level)
    for (int64_t j = 0; j < n; ++j)
      if (slice_level[j] < SLICE_NODE || slice_level[j] >= n_levels) return *bad = j, SLICE_BAD_LEVEL;
  if (slice_level)
    for (int64_t j = 0; j < n; ++j)
      if ((max_level ? max_level[j] : n_levels - 1) < slice_floor(slice_level[j])) return *bad = j, SLICE_BAD_MAX_LEVEL;
  return SLICE_OK;
}

// The rows and picks of a validated batch.  A pick is packed into 64 bits: row < 2^31, the units wanted
// u = count / z in [1, 2^31), max_level < 4.
struct SlicePlan {
  std::vector<SliceRow> rows;
  std::vector<uint64_t> picks;
  std::vector<int32_t> row_of, pick_of;     // per job
  std::vector<int32_t> row_tab, pick_tab;   // the dedupes' tables
};
PE_SL_HD uint64_t slice_pick_key(uint32_t row, int32_t units, int32_t max_level) {
  return ((uint64_t)row << 33) | ((uint64_t)(uint32_t)units << 2) | (uint64_t)max_level;
}
PE_SL_HD uint32_t slice_pick_row(uint64_t key) { return (uint32_t)(key >> 33); }
PE_SL_HD int32_t slice_pick_units(uint64_t key) { return (int32_t)((key >> 2) & 0x7FFFFFFF); }
PE_SL_HD int32_t slice_pick_max_level(uint64_t key) { return (int32_t)(key & 3); }

// shape_of[j]: job j's distinct shape (cap_dedupe's numbering).
inline void slice_plan_build(SlicePlan& p, int64_t n, const int32_t* shape_of, const int32_t* count,
                             const int32_t* slice_size, const int32_t* slice_level, const int32_t* max_level,
                             int32_t n_levels) {
  p.rows.clear();
  p.picks.clear();
  auto row_at = [&](int64_t j) {
    return slice_row((uint32_t)shape_of[j], slice_size ? slice_size[j] : 1, slice_level ? slice_level[j] : 0);
  };
  first_seen(
      n, p.row_tab, p.row_of,
      [&](int64_t j) {
        const SliceRow r = row_at(j);
        return first_seen_mix(first_seen_mix(((uint64_t)r.shape << 32) | (uint32_t)r.z) ^ (uint64_t)(uint32_t)r.sl);
      },
      [&](int64_t j, int32_t u) { return p.rows[(size_t)u] == row_at(j); }, [&](int64_t j) { p.rows.push_back(row_at(j)); });
  auto key_at = [&](int64_t j) {
    return slice_pick_key((uint32_t)p.row_of[(size_t)j], count[j] / (slice_size ? slice_size[j] : 1),
                          max_level ? max_level[j] : n_levels - 1);
  };
  first_seen(
      n, p.pick_tab, p.pick_of, [&](int64_t j) { return first_seen_mix(key_at(j)); },
      [&](int64_t j, int32_t u) { return p.picks[(size_t)u] == key_at(j); }, [&](int64_t j) { p.picks.push_back(key_at(j)); });
}
#endif

}  // namespace pe

#endif  // PE_SLICE_PLAN_H_
