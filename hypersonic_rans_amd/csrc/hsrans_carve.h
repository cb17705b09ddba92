// hsrans_carve.h — the two things every entry that packs many parts into one buffer needs: offsets carved out of a buffer at an alignment,
// and the rule for which byte ranges of a call's members may share memory.  Host only: no HIP, nothing device-side, no other project header.
#ifndef HSRANS_CARVE_H
#define HSRANS_CARVE_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Regions of one buffer, one after the other: take() aligns the cursor (align: a power of two), returns it as the region's offset and moves it
// past the region; `at` is the unaligned end of what was taken so far, close() the aligned one (the size of a buffer that is itself carved again).
struct Carve
{
  size_t at = 0;
  size_t take(size_t bytes, size_t align = 256)
  {
    const size_t here = close(align);
    at = here + bytes;
    return here;
  }
  size_t close(size_t align = 256) { return at = (at + align - 1) & ~(align - 1); }
};

// A byte range [lo, hi) that a call's kernels write (an output) or only read (an input); lo == hi: empty.
struct Span
{
  uintptr_t lo, hi;
  bool write;
};
inline Span span_of(const void *p, size_t bytes, bool write) { return Span{(uintptr_t)p, (uintptr_t)p + bytes, write}; }
// what the entries ask of a buffer before they form its span: set and 16-byte aligned; p + bytes does not pass the end of the address space
inline bool aligned16(const void *p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }
inline bool wraps(const void *p, size_t bytes) { return (uintptr_t)p + bytes < (uintptr_t)p; }

// The overlap rule of every batch entry:
//   two writes never intersect; a write never intersects a read; reads may share.
// False exactly when two non-empty spans intersect and at least one of them is a write.  One sort by start and one sweep that keeps the
// furthest end of the writes and of the reads begun so far (a span meets an earlier one exactly when it starts below that one's end); the
// spans come back sorted.
inline bool spans_disjoint(std::vector<Span> &spans)
{
  std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
  uintptr_t write_hi = 0, read_hi = 0;
  for (const Span &sp : spans)
  {
    if (sp.lo >= sp.hi)
      continue;
    if (sp.lo < write_hi || (sp.write && sp.lo < read_hi))
      return false;
    uintptr_t &hi = sp.write ? write_hi : read_hi;
    hi = std::max(hi, sp.hi);
  }
  return true;
}

// Whether a span of `a` intersects a span of `b`, whatever either reads or writes (empty spans meet nothing): for two groups that the rule
// above would let share, both being reads, and that still must stay apart.  One sort of b by start with the furthest end so far beside it,
// then for every span of a a binary search for the spans of b that begin below its end; b comes back sorted.
inline bool spans_meet(const std::vector<Span> &a, std::vector<Span> &b)
{
  std::sort(b.begin(), b.end(), [](const Span &x, const Span &y) { return x.lo < y.lo; });
  std::vector<uintptr_t> reach(b.size()); // the furthest end among b[0 .. k]'s non-empty spans
  uintptr_t hi = 0;
  for (size_t k = 0; k < b.size(); k++)
    reach[k] = hi = b[k].lo < b[k].hi ? std::max(hi, b[k].hi) : hi;
  for (const Span &sp : a)
  {
    if (sp.lo >= sp.hi)
      continue;
    const size_t below = std::lower_bound(b.begin(), b.end(), sp.hi, [](const Span &x, uintptr_t end) { return x.lo < end; }) - b.begin();
    if (below != 0 && reach[below - 1] > sp.lo)
      return true;
  }
  return false;
}

#endif // HSRANS_CARVE_H
