// planes_shuffle.h — what the byte-plane kernels (the ten hsrans_planes*.hip units) share.  The in-register byte shuffles: 16 elements of W
// bytes as they lie in memory <-> 16 bytes of each of the W planes, with v_perm_b32 (a 4 x 4 byte transpose is 8 of them).  The small
// helpers of the table- and list-driven kernels: wave-uniform values as scalars, the global-address cast, the element-wide stores of a
// block whose output is not 16-byte aligned, the search of a task's row in a prefix of task counts, and the walk of the member tables
// (a workgroup's member and its place in it).  And, at the end, what one lane of a WHOLE-TENSOR split or merge does, with or without a
// base: split_lanes and merge_lanes, the body of the one-tensor kernels (hsrans_planes.hip, hsrans_planes_delta.hip) and of the
// table-driven ones (hsrans_planes_batch.hip, hsrans_planes_delta.hip; hsrans_planes_diff.hip takes them without a base, for its members
// that have none, and keeps its own bodies for the zigzag difference, split_lanes_diff and merge_lanes_diff).  Device code only; every function is inlined into the kernel that
// calls it.  Everything is in hsrans::planes_detail; every unit says `using namespace`.
// (Sharing the whole-tensor body left the five table-driven kernels instruction for instruction as they were.  The one-tensor kernels
// came out 3 to 5 instructions shorter: with the plane pointers handed over by reference the compiler reads the kernel arguments once, on
// entry, where each kernel's own copy read them block by block and again in the tail; loads, v_perm_b32, XORs and stores are the same, in
// the same order.  The tail flag as a callable evaluated in the tail, or the pointers in a local array, gave the same kind of difference,
// never identity.  The six splits took it at no cost.  The merges did not, on 128 MiB against the written-out form: k_planes_merge<W> as
// a call to merge_lanes<W, false> 58.5 against 57.1 µs at W = 2, 66.8 against 66.2 at 4, 75.0 against 74.0 at 8 (medians of 48, three
// rounds; k_planes_merge<8> at 52 VGPRs for 51), k_planes_merge_delta<4> as a call to merge_lanes<4, true> 85.6 against 84.6 µs (medians of
// 96, three rounds; W = 2 and 8 level).  So k_planes_merge<W> and k_planes_merge_delta<W> keep merge_lanes written out, each in its unit:
// what merge_lanes says about the in-place order holds for k_planes_merge_delta's copy word for word.)
//
// What is NOT here: the range merges' 16-element block body — from the full-block path (load16 per plane, merge16, the 16-byte or
// element-wide stores) down to the byte-by-byte head and tail — which each of the four hsrans_planes_gather*.hip units writes out, and
// k_planes_merge_ranges_delta (hsrans_planes_delta.hip) a fifth time with the base.  As one __forceinline__ template (plane pointers by
// array reference or in a by-value struct, the output pointer __restrict__ or not) it changed the kernels' code every time: with
// __restrict__ k_planes_merge_ranges<2> went from 20 to 38 VGPRs and its unit from 513 to 688 instructions, and in all four forms the
// stores to a misaligned destination were merged differently in every kernel (fewer dwordx4, more dword and dwordx2).  Tried once more
// with the base as `merge_block<W, kDelta>(src[W], bsrc, out, base, lo, hi)` across all five: every kernel but k_planes_merge_indirect<2>
// and the cut changed, and grew — k_planes_merge_ranges<4> 162 -> 170 instructions, k_planes_merge_ranges_delta<4> 196 -> 211,
// k_planes_merge_ranges_batch 783 -> 788.  Nobody has measured what that costs, so the five copies stay until somebody does.
// A sixth, merge_block<W, kDelta>, lives in hsrans_planes_gather_delta.hip and is shared by that unit's three kernels, which were new with it.
#ifndef HSRANS_PLANES_SHUFFLE_H
#define HSRANS_PLANES_SHUFFLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsrans_planes.h"

namespace hsrans
{
namespace planes_detail
{
inline constexpr uint32_t kThreads = 256;     // lanes of a workgroup of every byte-plane kernel
inline constexpr uint32_t kLaneElements = 16; // elements a lane moves

// a value that is the same on every lane, moved to a scalar register
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v); }
// an address that came out of memory (a record's pointer) or was formed from one: that it is to device memory the compiler cannot see, so
// it is made a pointer to the global address space first and is addressed through with global_ instead of flat_ instructions
__device__ __forceinline__ uint8_t *global_at(uint64_t address)
{
  typedef __attribute__((address_space(1))) uint8_t global_u8;
  return (uint8_t *)(global_u8 *)address;
}

// the row of task t in the exclusive prefix of n rows' task counts: the last r with first_task[r] <= t (first_task[0] is 0 and t is below
// the total; rows without tasks share their successor's entry and are passed over).  A binary search that is the same on every lane.
__device__ __forceinline__ uint32_t task_row(const uint32_t *__restrict__ first_task, uint32_t n, uint32_t t)
{
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (uni(first_task[mid]) <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// ---- the member tables of hsrans_planes_batch.hip and hsrans_planes_delta.hip: one workgroup per task ----
// a pointer read from a record, the same on every lane
__device__ __forceinline__ uint8_t *uni_ptr(const uint8_t *p) { return global_at(uni64((uint64_t)p)); }
// the plain record of a table's record
__device__ __forceinline__ const PlanesBatchMember &batch_member(const PlanesBatchMember &r) { return r; }
__device__ __forceinline__ const PlanesBatchMember &batch_member(const PlanesDeltaBatchMember &r) { return r.m; }
// the record of task t: the last one with first_task <= t (first_task[0] is 0 and t is below the table's total); task_row's search over a
// field of the records
template <typename Record>
__device__ __forceinline__ const Record *member_of(const Record *__restrict__ members, uint32_t count, uint32_t t)
{
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (uni(batch_member(members[mid]).first_task) <= t)
      lo = mid;
    else
      hi = mid;
  }
  return members + lo;
}
// What one workgroup sees of its member: its index among the member's workgroups, whether it is the last of them, and the lane's 16 elements
struct Task
{
  uint64_t n, whole, lane;
  bool last;
};
__device__ __forceinline__ Task task_of(const PlanesBatchMember *m)
{
  Task t;
  t.n = uni64(m->n);
  t.whole = t.n / kLaneElements;
  const uint32_t block = blockIdx.x - uni(m->first_task);
  t.lane = (uint64_t)block * kThreads + threadIdx.x;
  t.last = block + 1 == planes_tasks_of(t.n);
  return t;
}

// __builtin_amdgcn_perm(hi, lo, sel): result byte k = byte sel[k] of {lo: 0..3, hi: 4..7}
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// 4 x 4 byte transpose: o[p] = {x0.byte p, x1.byte p, x2.byte p, x3.byte p} (its own inverse)
__device__ __forceinline__ void transpose4(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t o[4])
{
  const uint32_t a = perm(x1, x0, 0x05010400u), b = perm(x1, x0, 0x07030602u); // {x0.0, x1.0, x0.1, x1.1}, {x0.2, x1.2, x0.3, x1.3}
  const uint32_t c = perm(x3, x2, 0x05010400u), d = perm(x3, x2, 0x07030602u);
  o[0] = perm(c, a, 0x05040100u);
  o[1] = perm(c, a, 0x07060302u);
  o[2] = perm(d, b, 0x05040100u);
  o[3] = perm(d, b, 0x07060302u);
}

__device__ __forceinline__ void load16(const uint8_t *at, uint32_t *w)
{
  const uint4 v = *(const uint4 *)at;
  w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
}
__device__ __forceinline__ void store16(uint8_t *at, const uint32_t *w) { *(uint4 *)at = make_uint4(w[0], w[1], w[2], w[3]); }

// e[4 W]: 16 elements as they lie in memory, to `at` (a multiple of W, not of 16) as 16 element-wide stores
template <uint32_t W>
__device__ __forceinline__ void store_elements(uint8_t *at, const uint32_t *e)
{
#pragma unroll
  for (uint32_t i = 0; i < kLaneElements; i++)
  {
    if constexpr (W == 2)
      *(uint16_t *)(at + 2 * i) = (uint16_t)(e[i / 2] >> (16 * (i % 2)));
    else if constexpr (W == 4)
      *(uint32_t *)(at + 4 * i) = e[i];
    else
      *(uint2 *)(at + 8 * i) = make_uint2(e[2 * i], e[2 * i + 1]);
  }
}

// e[4 W]: 16 elements as they lie in memory; pl[p][j]: bytes 4 j .. 4 j + 3 of plane p's 16
template <uint32_t W>
__device__ __forceinline__ void split16(const uint32_t *e, uint32_t pl[W][4])
{
  if constexpr (W == 2)
  {
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
    {
      pl[0][j] = perm(e[2 * j + 1], e[2 * j], 0x06040200u);
      pl[1][j] = perm(e[2 * j + 1], e[2 * j], 0x07050301u);
    }
  }
  else
  {
    constexpr uint32_t DW = W / 4; // dwords per element: dword h of element i holds its bytes 4 h .. 4 h + 3
#pragma unroll
    for (uint32_t h = 0; h < DW; h++)
#pragma unroll
      for (uint32_t j = 0; j < 4; j++)
      {
        uint32_t o[4];
        transpose4(e[(4 * j) * DW + h], e[(4 * j + 1) * DW + h], e[(4 * j + 2) * DW + h], e[(4 * j + 3) * DW + h], o);
#pragma unroll
        for (uint32_t p = 0; p < 4; p++)
          pl[4 * h + p][j] = o[p];
      }
  }
}

template <uint32_t W>
__device__ __forceinline__ void merge16(const uint32_t pl[W][4], uint32_t *e)
{
  if constexpr (W == 2)
  {
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
    {
      e[2 * j] = perm(pl[1][j], pl[0][j], 0x05010400u);
      e[2 * j + 1] = perm(pl[1][j], pl[0][j], 0x07030602u);
    }
  }
  else
  {
    constexpr uint32_t DW = W / 4;
#pragma unroll
    for (uint32_t h = 0; h < DW; h++)
#pragma unroll
      for (uint32_t j = 0; j < 4; j++)
      {
        uint32_t o[4];
        transpose4(pl[4 * h][j], pl[4 * h + 1][j], pl[4 * h + 2][j], pl[4 * h + 3][j], o);
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
          e[(4 * j + i) * DW + h] = o[i];
      }
  }
}

// ---- the whole-tensor split and merge: what one lane does, for every kernel that moves whole tensors (k_planes_split / _merge<W> of
// hsrans_planes.hip, their delta forms and the table-driven kernels of hsrans_planes_batch.hip and hsrans_planes_delta.hip) ----
// n: the tensor's elements; whole: n / 16; lane: the lane's index among the tensor's lanes (its 16 elements are 16 lane ..); last: this is
// the tensor's last workgroup, whose first n % 16 lanes move the tail byte by byte, one element each.  planes: anything indexed 0 .. W - 1.
// kDelta: what enters the planes is in ^ base, what leaves them is XORed with the base again; without it `base` is not looked at.
template <uint32_t W, bool kDelta, typename Planes>
__device__ __forceinline__ void split_lanes(const uint8_t *in, const uint8_t *base, const Planes &planes, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(in + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
    if constexpr (kDelta)
    {
      uint32_t b[4 * W];
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
#pragma unroll
      for (uint32_t k = 0; k < 4 * W; k++)
        e[k] ^= b[k];
    }
    split16<W>(e, pl);
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      store16(planes[p] + lane * kLaneElements, pl[p]);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
    {
      if constexpr (kDelta)
        planes[p][i] = in[i * W + p] ^ base[i * W + p];
      else
        planes[p][i] = in[i * W + p];
    }
  }
}

// IN PLACE: with kDelta `out` may be `base` itself, so neither is __restrict__ here or in a kernel that passes them.  What makes that safe
// is the order below and nothing else: a lane loads ALL of its base bytes before its first store, in the tail the base byte is read and
// then the output byte is written, and no lane reads a byte another lane writes.
template <uint32_t W, bool kDelta, typename Planes>
__device__ __forceinline__ void merge_lanes(const Planes &planes, const uint8_t *base, uint8_t *out, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], b[kDelta ? 4 * W : 1], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(planes[p] + lane * kLaneElements, pl[p]);
    if constexpr (kDelta)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    }
    merge16<W>(pl, e);
    if constexpr (kDelta)
    {
#pragma unroll
      for (uint32_t k = 0; k < 4 * W; k++)
        e[k] ^= b[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      store16(out + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
    {
      uint8_t b = 0;
      if constexpr (kDelta)
        b = base[i * W + p];
      out[i * W + p] = planes[p][i] ^ b;
    }
  }
}
} // namespace planes_detail
} // namespace hsrans

#endif // HSRANS_PLANES_SHUFFLE_H
