// The host side of pe_gang_split_tree and the one piece of arithmetic it shares with tree_split_kernel
// (pe_split.hip).  Plain C++, no HIP: the engine includes it on the host, the kernel for split_tr, and
// tests/cpp/test_split_plan.cc builds it under the sanitizers.
//
// The descent's step for one parent with allotment a, in its threshold form (include/placement.h states the
// walk): with H(v) = the sum of the child slots >= v and G(v) = the sum of those > v, let v* be the largest
// child value with H(v*) >= a.  The whole parts are the children above v* and the first t children equal
// to v* in id order, the last part gets r pods: split_tr.
//
// The device answers the picks of a call -- its distinct (shape, count, max_level) -- one slice at a time,
// into one buffer of int32 words per slice (SplitLayout):
//   part domains [n][max_parts] | parts [n], spread [n][4] | part pods [n][max_parts]
// The small block sits in the middle, so whatever subset of the outputs the caller asked for is one
// contiguous range (split_copy_range) and crosses with one copy.  A slice holds as many picks as keep the
// buffer within SPLIT_BUFFER_BYTES, the bound of the capacity tables (split_slice_picks).
#ifndef PE_SPLIT_PLAN_H_
#define PE_SPLIT_PLAN_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PE_SP_HD __host__ __device__ __forceinline__
#elif defined(__HIPCC__)
#define PE_SP_HD __host__ __device__ inline
#else
#define PE_SP_HD inline
#endif

namespace pe {

constexpr int SPLIT_MAX_PARTS = 1024;   // PE_MAX_SPLIT_PARTS
constexpr int SPLIT_TOO_MANY = -1;      // PE_SPLIT_TOO_MANY
constexpr int SPLIT_LEVELS = 4;         // PE_MAX_LEVELS: a pick's spread row
constexpr int SPLIT_META_WORDS = 1 + SPLIT_LEVELS;   // parts, spread[4]
constexpr int64_t SPLIT_BUFFER_BYTES = int64_t(64) << 20;

// t and r of a parent's step: a = the allotment (>= 1), G = the sum of the child slots above v, v = v* (>= 1),
// with G < a <= G + (number of children equal to v) * v.  t = ceil((a - G) / v) - 1 and r = a - G - t * v,
// so 0 < r <= v.  All values stay below 2^56.
struct SplitTR {
  uint64_t t, r;
};
PE_SP_HD SplitTR split_tr(uint64_t a, uint64_t G, uint64_t v) {
  const uint64_t rem = a - G;   // >= 1
  if (rem <= v) return SplitTR{0, rem};
  const uint64_t t = (rem - 1) / v;
  return SplitTR{t, rem - t * v};
}

// int32 words and bytes of one pick's row in the slice buffer
PE_SP_HD int64_t split_row_words(int32_t max_parts) { return 2 * (int64_t)max_parts + SPLIT_META_WORDS; }
PE_SP_HD int64_t split_row_bytes(int32_t max_parts) { return split_row_words(max_parts) * (int64_t)sizeof(int32_t); }

// Picks per slice: the most whose rows stay within SPLIT_BUFFER_BYTES (8172 at least: max_parts <= 1024).
PE_SP_HD int64_t split_slice_picks(int32_t max_parts) { return SPLIT_BUFFER_BYTES / split_row_bytes(max_parts); }

// Where the three blocks of a slice of n picks begin, in int32 words.
struct SplitLayout {
  int64_t n;
  int32_t max_parts;
  PE_SP_HD int64_t dom_at() const { return 0; }
  PE_SP_HD int64_t meta_at() const { return n * max_parts; }
  PE_SP_HD int64_t pods_at() const { return meta_at() + n * SPLIT_META_WORDS; }
  PE_SP_HD int64_t words() const { return pods_at() + n * max_parts; }
};

// The smallest word range [first, first + count) that holds the blocks asked for; count 0 when none is.
struct SplitRange {
  int64_t first, count;
};
PE_SP_HD SplitRange split_copy_range(const SplitLayout& L, bool dom, bool meta, bool pods) {
  if (!dom && !meta && !pods) return SplitRange{0, 0};
  const int64_t b = dom ? L.dom_at() : (meta ? L.meta_at() : L.pods_at());
  const int64_t e = pods ? L.words() : (meta ? L.pods_at() : L.meta_at());
  return SplitRange{b, e - b};
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The scatter from a slice's picks to the jobs [j0, j1) (jobs are independent: ranges may run on threads of
// their own).  `buf` is the slice buffer as it lay on the device (only the copied range need be valid),
// pick_of[j] the pick of job j, [p0, p0 + L.n) the slice; live(p) says whether the launch answered pick p (its
// shape lay in the launch's chunk of shapes).  Each output may be NULL; rows are [max_parts] (parts) and
// [n_levels] (spread) per job.
template <class Live>
inline void split_scatter(const int32_t* buf, const SplitLayout& L, int64_t p0, int64_t j0, int64_t j1, const int32_t* pick_of,
                          int32_t n_levels, Live live, int32_t* out_parts, int32_t* out_part_domain,
                          int32_t* out_part_pods, int32_t* out_spread) {
  const int64_t mp = L.max_parts;
  for (int64_t j = j0; j < j1; ++j) {
    const int64_t p = pick_of[j], k = p - p0;
    if (k < 0 || k >= L.n || !live(p)) continue;
    const int32_t* meta = buf + L.meta_at() + k * SPLIT_META_WORDS;
    if (out_parts) out_parts[j] = meta[0];
    if (out_spread)
      for (int32_t l = 0; l < n_levels; ++l) out_spread[j * n_levels + l] = meta[1 + l];
    if (out_part_domain) memcpy(out_part_domain + j * mp, buf + L.dom_at() + k * mp, (size_t)mp * sizeof(int32_t));
    if (out_part_pods) memcpy(out_part_pods + j * mp, buf + L.pods_at() + k * mp, (size_t)mp * sizeof(int32_t));
  }
}
#endif

}  // namespace pe

#endif  // PE_SPLIT_PLAN_H_
