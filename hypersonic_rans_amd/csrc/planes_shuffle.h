// planes_shuffle.h — what the byte-plane kernels (the ten hsrans_planes*.hip units) share.  The in-register byte shuffles: 16 elements of W
// bytes as they lie in memory <-> 16 bytes of each of the W planes, with v_perm_b32 (a 4 x 4 byte transpose is 8 of them).  The small
// helpers of the table- and list-driven kernels: wave-uniform values as scalars, the global-address cast, the element-wide stores of a
// block whose output is not 16-byte aligned, the search of a task's row in a prefix of task counts, and the walk of the member tables
// (a workgroup's member and its place in it).  The residue rules as types — RuleNone, RuleXor, RuleDiff: what a tensor coded against a
// base leaves in its planes, as a step on a full block's words and a step on one element.  And, at the end, what one lane of a
// WHOLE-TENSOR split or merge does under a rule: split_lanes<W, Rule> and merge_lanes<W, Rule>, the body of the one-tensor kernels
// (hsrans_planes.hip, hsrans_planes_base.hip) and of the table-driven ones (hsrans_planes_batch.hip, hsrans_planes_base.hip).  Device code
// only; every function is inlined into the kernel that calls it.  Everything is in hsrans::planes_detail; every unit says `using namespace`.
//
// What was measured, and what it decided (128 MiB, medians over three rounds; CHANGELOG.md has the runs):
// - The splits and the table-driven kernels took the shared body at no cost.  The one-tensor merges did not: as a call to merge_lanes the
//   kernel reads all its arguments on entry, comes out 3 to 5 instructions shorter and is slower — k_planes_merge<W> 58.5 against 57.1 µs
//   at W = 2, 66.8 against 66.2 at 4, 75.0 against 74.0 at 8 (k_planes_merge<8> at 52 VGPRs for 51), k_planes_merge_delta<4> 85.6 against
//   84.6 µs (75 / 135 / 231 instructions for 80 / 139 / 235).  So k_planes_merge<W> and k_planes_merge_delta<W> keep merge_lanes written
//   out, each in its unit; what merge_lanes says about the in-place order holds for k_planes_merge_delta's copy word for word.
//   k_planes_merge_diff<W> was born as the call and stays one.
// - With the rule as a type in place of a `bool kDelta` and a forked pair of diff bodies, every kernel of hsrans_planes.hip and
//   hsrans_planes_batch.hip and the 16 whole-tensor and table-driven kernels of hsrans_planes_base.hip are instruction for instruction what
//   they were.  Three things that took: the element steps get the tensors' pointers and an index (a pointer to the element changed the
//   tails), merge_element keeps the caller's index type, and each rule's merge_element reads in the order its tail had.
//
// What is NOT here: the range merges' 16-element block body — from the full-block path (load16 per plane, merge16, the 16-byte or
// element-wide stores) down to the head and tail — which each of the four hsrans_planes_gather*.hip units writes out, and
// hsrans_planes_base.hip twice more with the base, k_planes_merge_ranges_delta and k_planes_merge_ranges_diff.  As one __forceinline__
// template (plane pointers by array reference or in a by-value struct, the output pointer __restrict__ or not, with or without the base)
// it changed the kernels' code every time, and grew it: with __restrict__ k_planes_merge_ranges<2> went from 20 to 38 VGPRs, with the
// base k_planes_merge_ranges<4> 162 -> 170 instructions, k_planes_merge_ranges_delta<4> 196 -> 211, k_planes_merge_ranges_batch 783 -> 788,
// and the stores to a misaligned destination were merged differently in every kernel.  Even the rule's name is enough: with the full
// block's step spelled Rule::restore_words the two copies with a base came out at 125 / 196 / 322 instructions for 127 / 196 / 322 (XOR,
// all three changed) and 155 / 255 / 384 for 155 / 255 / 378 (diff, the last changed).  Nobody has measured what any of that costs, so
// the six copies stay as they were until somebody does.  A seventh, merge_block<W, Rule>, lives in hsrans_planes_gather_delta.hip and is
// shared by that unit's three kernels, which were new with it; it says itself what the rule's steps did to them.
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

// ---- the member tables of hsrans_planes_batch.hip and hsrans_planes_base.hip: one workgroup per task ----
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

// ---- the residue rules: what a tensor coded against a base leaves in its planes (PlanesRule, hsrans_planes.h), as types ----
// RuleNone: no base, the planes hold the elements' bytes.  RuleXor: in ^ base.  RuleDiff: with an element read as a little-endian unsigned
// integer of W bytes and all arithmetic modulo 2^(8 W),
//   split:  d = in - base,  z = (d << 1) ^ (0 - (d >> (8 W - 1)))        merge:  d = (z >> 1) ^ (0 - (z & 1)),  out = base + d
// — the wrapped difference with its sign folded into the lowest bit.  Exactly invertible for every bit pattern; nothing is read as a float.
// Each rule has kBase (whether the base is looked at at all), the step on the e[] words of a full block — e[4 W], b[4 W]: 16 elements and
// their base's as they lie in memory, in front of split16 (residue_words) or behind merge16 (restore_words); a lane owns 16 whole elements,
// so no carry ever leaves a lane — and the step on ONE element, for tails and the range merges' heads and tails:
//   split_element<W>(in, base, planes, i)            planes[p][i] from element i of in and base
//   merge_element<W>(planes, i, base, bi, out, oi)   element oi of out from byte i of the planes and element bi of base
// The element steps take the tensors' pointers and an index, never a pointer to the element (that changed the tails' code); i and bi keep
// the caller's index type (the whole-tensor tails count in uint64_t, the range merges in uint32_t).
// IN PLACE: `out` may be `base`.  Every merge_element reads its base bytes BEFORE it writes: RuleXor the base byte, then the plane byte,
// then the store; RuleDiff the base element, then z from the plane bytes, then the store.  A new rule must keep that order.
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

// e becomes z (split): a word holds two 2-byte elements (packed 16-bit operations on a two-element vector), one 4-byte element (plain
// 32-bit) or half an 8-byte element (the two words joined for one 64-bit subtract) ...
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

struct RuleNone
{
  static constexpr bool kBase = false;
  template <uint32_t W>
  static __device__ __forceinline__ void residue_words(uint32_t *, const uint32_t *)
  {
  }
  template <uint32_t W>
  static __device__ __forceinline__ void restore_words(uint32_t *, const uint32_t *)
  {
  }
  template <uint32_t W, typename Planes>
  static __device__ __forceinline__ void split_element(const uint8_t *in, const uint8_t *, const Planes &planes, uint64_t i)
  {
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      planes[p][i] = in[i * W + p];
  }
  template <uint32_t W, typename Planes, typename Index>
  static __device__ __forceinline__ void merge_element(const Planes &planes, Index i, const uint8_t *, Index, uint8_t *out, uint64_t oi)
  {
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      out[oi * W + p] = planes[p][i];
  }
};

struct RuleXor
{
  static constexpr bool kBase = true;
  template <uint32_t W>
  static __device__ __forceinline__ void residue_words(uint32_t *e, const uint32_t *b)
  {
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
      e[k] ^= b[k];
  }
  template <uint32_t W>
  static __device__ __forceinline__ void restore_words(uint32_t *e, const uint32_t *b)
  {
    residue_words<W>(e, b);
  }
  template <uint32_t W, typename Planes>
  static __device__ __forceinline__ void split_element(const uint8_t *in, const uint8_t *base, const Planes &planes, uint64_t i)
  {
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      planes[p][i] = in[i * W + p] ^ base[i * W + p];
  }
  template <uint32_t W, typename Planes, typename Index>
  static __device__ __forceinline__ void merge_element(const Planes &planes, Index i, const uint8_t *base, Index bi, uint8_t *out, uint64_t oi)
  {
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
    {
      const uint8_t b = base[bi * W + p];
      out[oi * W + p] = planes[p][i] ^ b;
    }
  }
};

struct RuleDiff
{
  static constexpr bool kBase = true;
  template <uint32_t W>
  static __device__ __forceinline__ void residue_words(uint32_t *e, const uint32_t *b)
  {
    diff_words<W>(e, b);
  }
  template <uint32_t W>
  static __device__ __forceinline__ void restore_words(uint32_t *e, const uint32_t *b)
  {
    undiff_words<W>(e, b);
  }
  template <uint32_t W, typename Planes>
  static __device__ __forceinline__ void split_element(const uint8_t *in, const uint8_t *base, const Planes &planes, uint64_t i)
  {
    const typename ElementOf<W>::type z = zigzag_of(element_at<W>(in, i), element_at<W>(base, i));
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      planes[p][i] = (uint8_t)(z >> (8 * p));
  }
  template <uint32_t W, typename Planes, typename Index>
  static __device__ __forceinline__ void merge_element(const Planes &planes, Index i, const uint8_t *base, Index bi, uint8_t *out, uint64_t oi)
  {
    const typename ElementOf<W>::type b = element_at<W>(base, bi);
    *(typename ElementOf<W>::type *)(out + oi * W) = undo_zigzag(z_at<W>(planes, i), b);
  }
};

// ---- the whole-tensor split and merge: what one lane does, for every kernel that moves whole tensors (k_planes_split / _merge<W> of
// hsrans_planes.hip, the forms with a base and the table-driven kernels of hsrans_planes_batch.hip and hsrans_planes_base.hip) ----
// n: the tensor's elements; whole: n / 16; lane: the lane's index among the tensor's lanes (its 16 elements are 16 lane ..); last: this is
// the tensor's last workgroup, whose first n % 16 lanes move the tail, one element each.  planes: anything indexed 0 .. W - 1.
// Rule: what enters the planes, and how it leaves them; with RuleNone `base` is not looked at.
template <uint32_t W, typename Rule, typename Planes>
__device__ __forceinline__ void split_lanes(const uint8_t *in, const uint8_t *base, const Planes &planes, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], b[Rule::kBase ? 4 * W : 1], pl[W][4];
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(in + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
    if constexpr (Rule::kBase)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    }
    Rule::template residue_words<W>(e, b);
    split16<W>(e, pl);
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      store16(planes[p] + lane * kLaneElements, pl[p]);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
    Rule::template split_element<W>(in, base, planes, whole * kLaneElements + threadIdx.x);
}

// IN PLACE: with a base `out` may be `base` itself, so neither is __restrict__ here or in a kernel that passes them.  What makes that safe
// is the order below and nothing else, under every rule: a lane loads ALL of its base bytes before its first store, in the tail the base is
// read and then the output is written (each rule's merge_element keeps that order, as said above), and no lane reads a byte another lane writes.
template <uint32_t W, typename Rule, typename Planes>
__device__ __forceinline__ void merge_lanes(const Planes &planes, const uint8_t *base, uint8_t *out, uint64_t n, uint64_t whole, uint64_t lane, bool last)
{
  if (lane < whole)
  {
    uint32_t e[4 * W], b[Rule::kBase ? 4 * W : 1], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(planes[p] + lane * kLaneElements, pl[p]);
    if constexpr (Rule::kBase)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    }
    merge16<W>(pl, e);
    Rule::template restore_words<W>(e, b);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      store16(out + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (last && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
    Rule::template merge_element<W>(planes, i, base, i, out, i);
  }
}
} // namespace planes_detail
} // namespace hsrans

#endif // HSRANS_PLANES_SHUFFLE_H
