// libplacement: the layout of a domain call's pinned blocks (pe_ctx.h dm_hin / dm_in and dm_out / dm_hout), stated
// once.  A call adds its parts in the order they lie in the block and gets typed offsets back; the same part then
// addresses the pinned copy, the device copy and the read-back.  Every part starts at a multiple of its type's
// alignment or of a larger one the call names, whatever the order of the parts.  Host-only: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>

namespace pe {

// `count` elements of T at byte `at` of a block; count == 0: an empty part, which still has its place.
template <class T>
struct BlockPart {
  size_t at = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
  size_t end() const { return at + bytes(); }
  T* in(uint8_t* base) const { return reinterpret_cast<T*>(base + at); }
  const T* in(const uint8_t* base) const { return reinterpret_cast<const T*>(base + at); }
};

struct BlockLayout {
  size_t end = 0, lo = 0, hi = 0;   // the end of the last part; [lo, hi): from the first wanted part to the end of
  bool any = false;                 // the last, the one copy out -- where any part is wanted at all
  size_t bytes() const { return end; }
  // The next part: behind the last one, rounded up to max(alignof(T), align); align: a power of two.  wanted: the
  // part is to come back (the caller's output pointer is there, or a flag such as ev.on is set).
  template <class T>
  BlockPart<T> add(int64_t count, size_t align = alignof(T), bool wanted = false) {
    const size_t a = align > alignof(T) ? align : alignof(T);
    const BlockPart<T> part{(end + a - 1) & ~(a - 1), (size_t)count};
    end = part.end();
    if (wanted) {
      if (!any || part.at < lo) lo = part.at;
      if (!any || part.end() > hi) hi = part.end();
      any = true;
    }
    return part;
  }
};

}  // namespace pe
