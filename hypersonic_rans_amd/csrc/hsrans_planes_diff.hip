// hsrans_planes_diff.hip — the byte-plane kernels for a tensor coded against a base as a zigzag DIFFERENCE (hsrans_*_device_planes_diff).
// Where the delta kernels (hsrans_planes_delta.hip) put in ^ base into the planes, these put z there: with an element read as a
// little-endian unsigned integer of W bytes and all arithmetic modulo 2^(8 W),
//   split:  d = in - base,  z = (d << 1) ^ (0 - (d >> (8 W - 1)))        merge:  d = (z >> 1) ^ (0 - (z & 1)),  out = base + d
// — the wrapped difference with its sign folded into the lowest bit, so that a base a few ulps away leaves small bytes in every plane where
// the XOR leaves 2^(k+1) - 1 for a carry through k bits.  Exactly invertible for every bit pattern; nothing is read as a float.
// The kernels mirror that unit's one for one: k_planes_split_diff<W>, k_planes_merge_diff<W>, the table-driven k_planes_split_diff_batch and
// k_planes_merge_diff_batch over the same PlanesDeltaBatchMember records (a null base: the member goes as it is, by split_lanes /
// merge_lanes without a base, planes_shuffle.h), and k_planes_merge_ranges_diff<W> with the base read at the SOURCE element's index.
// Full blocks.  A lane owns 16 whole elements, so no carry ever leaves a lane.  The rule is applied on the e[] words — 16 elements as they
// lie in memory, behind merge16 or in front of split16: a word holds two 2-byte elements (packed 16-bit operations on a two-element
// vector), one 4-byte element (plain 32-bit) or half an 8-byte element (the two words joined for one 64-bit add or subtract).
// Tails, and the range merge's heads and tails, go per ELEMENT, not per byte: a lane assembles its element from the W plane bytes, reads
// the base's element, applies the rule and writes the element (the split: its W bytes).
// In place.  The whole-tensor merges take out == base: neither is __restrict__, and what makes it safe is the order of merge_lanes
// (planes_shuffle.h), kept by merge_lanes_diff below: ALL of a lane's base loads come before its first store, in the tail the base element
// is read and then the output element is written, and no lane reads a byte another lane writes.  Partial overlap is not safe, and the
// entries refuse it.
// No LDS, no scratch.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

namespace hsrans
{
namespace
{
using namespace planes_detail;

// ---- the rule ----
template <uint32_t W>
struct ElementOf;
template <>
struct ElementOf<2>
{
  typedef uint16_t type;
};
template <>
struct ElementOf<4>
{
  typedef uint32_t type;
};
template <>
struct ElementOf<8>
{
  typedef uint64_t type;
};

// one element (T: unsigned, 2, 4 or 8 bytes; the casts take back what integer promotion widens)
template <typename T>
__device__ __forceinline__ T zigzag_of(T in, T base)
{
  const T d = (T)(in - base);
  return (T)((T)(d << 1) ^ (T)((T)0 - (T)(d >> (8 * sizeof(T) - 1))));
}
template <typename T>
__device__ __forceinline__ T undo_zigzag(T z, T base)
{
  const T d = (T)((T)(z >> 1) ^ (T)((T)0 - (T)(z & 1)));
  return (T)(base + d);
}

// two 2-byte elements in one word: component 0 is the word's low half, the element that lies first in memory
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// e[4 W], b[4 W]: 16 elements and their base's as they lie in memory; e becomes z (split) ...
template <uint32_t W>
__device__ __forceinline__ void diff_words(uint32_t *e, const uint32_t *b)
{
  if constexpr (W == 2)
  {
    const u16x2 zero = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
    {
      const u16x2 d = __builtin_bit_cast(u16x2, e[k]) - __builtin_bit_cast(u16x2, b[k]);
      e[k] = __builtin_bit_cast(uint32_t, (u16x2)((d << 1) ^ (zero - (d >> 15))));
    }
  }
  else if constexpr (W == 4)
  {
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
      e[k] = zigzag_of<uint32_t>(e[k], b[k]);
  }
  else
  {
#pragma unroll
    for (uint32_t i = 0; i < kLaneElements; i++)
    {
      const uint64_t z = zigzag_of<uint64_t>(((uint64_t)e[2 * i + 1] << 32) | e[2 * i], ((uint64_t)b[2 * i + 1] << 32) | b[2 * i]);
      e[2 * i] = (uint32_t)z, e[2 * i + 1] = (uint32_t)(z >> 32);
    }
  }
}
// ... and e, holding z, becomes the elements (merge)
template <uint32_t W>
__device__ __forceinline__ void undiff_words(uint32_t *e, const uint32_t *b)
{
  if constexpr (W == 2)
  {
    const u16x2 zero = {0, 0}, one = {1, 1};
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
    {
      const u16x2 z = __builtin_bit_cast(u16x2, e[k]);
      const u16x2 d = (z >> 1) ^ (zero - (z & one));
      e[k] = __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, b[k]) + d));
    }
  }
  else if constexpr (W == 4)
  {
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
      e[k] = undo_zigzag<uint32_t>(e[k], b[k]);
  }
  else
  {
#pragma unroll
    for (uint32_t i = 0; i < kLaneElements; i++)
    {
      const uint64_t v = undo_zigzag<uint64_t>(((uint64_t)e[2 * i + 1] << 32) | e[2 * i], ((uint64_t)b[2 * i + 1] << 32) | b[2 * i]);
      e[2 * i] = (uint32_t)v, e[2 * i + 1] = (uint32_t)(v >> 32);
    }
  }
}

// element i of a tensor of W-byte elements (the tensor 16-byte aligned: every element lies at a multiple of W)
template <uint32_t W>
__device__ __forceinline__ typename ElementOf<W>::type element_at(const uint8_t *elements, uint64_t i)
{
  return *(const typename ElementOf<W>::type *)(elements + i * W);
}
// z of element i, assembled from byte i of each of the W planes (anything indexed 0 .. W - 1)
template <uint32_t W, typename Planes>
__device__ __forceinline__ typename ElementOf<W>::type z_at(const Planes &planes, uint64_t i)
{
  typename ElementOf<W>::type z = 0;
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    z |= (typename ElementOf<W>::type)planes[p][i] << (8 * p);
  return z;
}

// ---- the whole-tensor split and merge: split_lanes and merge_lanes (planes_shuffle.h: n, whole, lane, last as there) under this rule ----
template <uint32_t W, typename Planes>
__device__ __forceinline__ void split_lanes_diff(const uint8_t *in, const uint8_t *base, const Planes &planes, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(in + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    diff_words<W>(e, b);
    split16<W>(e, pl);
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      store16(planes[p] + lane * kLaneElements, pl[p]);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
    const typename ElementOf<W>::type z = zigzag_of(element_at<W>(in, i), element_at<W>(base, i));
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      planes[p][i] = (uint8_t)(z >> (8 * p));
  }
}

// IN PLACE: `out` may be `base` itself, so neither is __restrict__ here or in a kernel that passes them.  The order is merge_lanes': a lane
// loads ALL of its base bytes before its first store; in the tail the base element is read and then the output element is written.
template <uint32_t W, typename Planes>
__device__ __forceinline__ void merge_lanes_diff(const Planes &planes, const uint8_t *base, uint8_t *out, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(planes[p] + lane * kLaneElements, pl[p]);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    merge16<W>(pl, e);
    undiff_words<W>(e, b);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      store16(out + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
    const typename ElementOf<W>::type b = element_at<W>(base, i);
    *(typename ElementOf<W>::type *)(out + i * W) = undo_zigzag(z_at<W>(planes, i), b);
  }
}

// ---- one tensor: the grids of hsrans_planes.hip ----
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_split_diff(const uint8_t *__restrict__ in, const uint8_t *__restrict__ base, uint64_t n, PlanePtrs planes)
{
  split_lanes_diff<W>(in, base, planes.p, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}

// (base and out may be the same buffer: not __restrict__)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_diff(PlanePtrs planes, const uint8_t *base, uint64_t n, uint8_t *out)
{
  merge_lanes_diff<W>(planes.p, base, out, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}

// ---- many tensors: the table walk of hsrans_planes_delta.hip over the same records ----
// kBase: the member has a base (decided per workgroup, from the record); without one it is split or merged as it is
template <uint32_t W, bool kBase>
__device__ __forceinline__ void split_task(const PlanesDeltaBatchMember *m)
{
  const Task t = task_of(&m->m);
  const uint8_t *in = uni_ptr(m->m.elements), *base = uni_ptr(m->base);
  uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->m.plane[p]);
  if constexpr (kBase)
    split_lanes_diff<W>(in, base, planes, t.n, t.whole, t.lane, t.last);
  else
    split_lanes<W, false>(in, base, planes, t.n, t.whole, t.lane, t.last);
}

template <uint32_t W, bool kBase>
__device__ __forceinline__ void merge_task(const PlanesDeltaBatchMember *m)
{
  const Task t = task_of(&m->m);
  uint8_t *out = uni_ptr(m->m.elements);
  const uint8_t *base = uni_ptr(m->base); // (may be `out`)
  const uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->m.plane[p]);
  if constexpr (kBase)
    merge_lanes_diff<W>(planes, base, out, t.n, t.whole, t.lane, t.last);
  else
    merge_lanes<W, false>(planes, base, out, t.n, t.whole, t.lane, t.last);
}

template <bool kBase>
__device__ __forceinline__ void split_member(const PlanesDeltaBatchMember *m, uint32_t W)
{
  if (W == 2)
    split_task<2, kBase>(m);
  else if (W == 4)
    split_task<4, kBase>(m);
  else if (W == 8)
    split_task<8, kBase>(m);
}
template <bool kBase>
__device__ __forceinline__ void merge_member(const PlanesDeltaBatchMember *m, uint32_t W)
{
  if (W == 2)
    merge_task<2, kBase>(m);
  else if (W == 4)
    merge_task<4, kBase>(m);
  else if (W == 8)
    merge_task<8, kBase>(m);
}

// grid: the table's task total; count: its records
__global__ __launch_bounds__(kThreads) void k_planes_split_diff_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesDeltaBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->m.W);
  if (uni64((uint64_t)m->base) != 0)
    split_member<true>(m, W);
  else
    split_member<false>(m, W);
}

__global__ __launch_bounds__(kThreads) void k_planes_merge_diff_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesDeltaBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->m.W);
  if (uni64((uint64_t)m->base) != 0)
    merge_member<true>(m, W);
  else
    merge_member<false>(m, W);
}

// ---- element ranges of one frame: k_planes_merge_ranges_delta's body (hsrans_planes_delta.hip) under this rule ----
static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements, "one lane per 16-element block of a task");

// grid: one workgroup per task; xbase: the whole base tensor, in the frame's element coordinates (never the output: __restrict__)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges_diff(PlanePtrs planes, uint32_t work_mask, const PlanesGatherTask *__restrict__ tasks,
                                                                       const uint8_t *__restrict__ xbase, uint8_t *__restrict__ out)
{
  const PlanesGatherTask t = tasks[blockIdx.x];
  const uint32_t first = threadIdx.x * kLaneElements; // the lane's block: elements [src + first, src + first + 16)
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements; // (t.lo < 16: only lane 0 has a head)
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    src[p] = planes.p[p] + (((work_mask >> p) & 1) != 0 ? t.work_pos : t.src) + first;
  const uint8_t *bsrc = xbase + (t.src + first) * W; // the block's base bytes: 16-byte aligned (src a multiple of 16 elements)
  const uint64_t base = t.src + first + (uint64_t)t.dst_delta; // the output element of the block's element 0 (modulo 2^64: a head's may lie below 0)
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(bsrc + 16 * k, b + 4 * k);
    merge16<W>(pl, e);
    undiff_words<W>(e, b);
    uint8_t *dst = out + base * W;
    if (((uintptr_t)dst & 15) == 0)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        store16(dst + 16 * k, e + 4 * k);
    }
    else
      store_elements<W>(dst, e);
    return;
  }
  for (uint32_t i = lo; i < hi; i++) // (base elements of the range's own elements only)
    *(typename ElementOf<W>::type *)(out + (base + i) * W) = undo_zigzag(z_at<W>(src, i), element_at<W>(bsrc, i));
}

} // namespace

// ---- the launches alone: launch_planes_split, _merge and _merge_ranges check the arguments and form the grid, and come here with a base
// and PlanesRule::kDiff ----
void planes_diff_split_kernel(uint32_t W, uint32_t grid, const uint8_t *in, const uint8_t *base, uint64_t n, const PlanePtrs &planes, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) { k_planes_split_diff<w()><<<grid, kThreads, 0, stream>>>(in, base, n, planes); });
}

void planes_diff_merge_kernel(uint32_t W, uint32_t grid, const PlanePtrs &planes, const uint8_t *base, uint64_t n, uint8_t *out, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) { k_planes_merge_diff<w()><<<grid, kThreads, 0, stream>>>(planes, base, n, out); });
}

void planes_diff_merge_ranges_kernel(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks, const uint8_t *base,
                                     uint8_t *out, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) { k_planes_merge_ranges_diff<w()><<<n_tasks, kThreads, 0, stream>>>(planes, work_mask, d_tasks, base, out); });
}

hipError_t launch_planes_split_diff_batch(const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  k_planes_split_diff_batch<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

hipError_t launch_planes_merge_diff_batch(const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  k_planes_merge_diff_batch<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

} // namespace hsrans
