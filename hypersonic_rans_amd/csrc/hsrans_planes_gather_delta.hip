// hsrans_planes_gather_delta.hip — the merges of the three gathers that undo a delta while they fetch
// (hsrans_decode_device_planes_gather_indirect_delta, _gather_batch_delta, _gather_batch_indirect_delta): what comes out of the planes is
// XORed with the base at the SOURCE element's index, as k_planes_merge_ranges_delta (hsrans_planes_base.hip) does for one frame and ranges
// on the host.  k_planes_merge_indirect_delta<W> is k_planes_merge_indirect<W> (hsrans_planes_gather_indirect.hip) with the base tensor as
// one more argument; k_planes_merge_ranges_batch_delta and k_planes_merge_batch_indirect_delta are k_planes_merge_ranges_batch
// (hsrans_planes_gather_batch.hip) and k_planes_merge_batch_indirect (hsrans_planes_gather_batch_indirect.hip) with a table of one base
// address per member beside the member records, 0 for a member that goes as it is.  The cuts, the task lists and the control workspaces
// are the plain calls': a base moves no row, no slot and no task.
// The range merges' block body is written ONCE here, merge_block<W, Rule>, for the three kernels (planes_shuffle.h says why the six
// earlier copies are not shared; these three were new with it, so nothing had to stay as it was).  Rule is the residue rule as a type
// (planes_shuffle.h): RuleNone for a member without a base, RuleXor with one.  The body still spells the XOR itself, in both places: with
// the full block's step as Rule::restore_words, k_planes_merge_indirect_delta<2> came out at 304 instructions for 306, the two table-driven
// kernels at 1768 for 1770 and 1909 for 1911 (one v_bfi_b32 that changes nothing and its constant gone; <4> and <8> as they were), and with
// the head's and tail's step as Rule::merge_element too all five changed (304, 406, 398, 1767, 1900 for 306, 406, 404, 1770, 1911).
// Nobody has measured either form, so neither is in; the diff forms of these gathers need both, and the measurement with them.
// No aliasing: a base is never an output, so both are __restrict__.
#include "hsrans_planes.h"
#include "hsrans_plan.h"
#include "planes_cut.h"
#include "planes_shuffle.h"

#include <algorithm>

namespace hsrans
{
namespace
{
using namespace planes_detail;

static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements && kPlanesCutTask == kPlanesGatherTaskElements, "one lane per 16-element block of a task");
static_assert(sizeof(PlanesGatherBatchTask) == 48 && sizeof(PlanesGatherBatchMember) == 72 && sizeof(PlanesRange) == 24 && sizeof(PlanesSetRow) == 32,
              "the task list's, the member table's, the ranges' and the rows' layout");

// ---------------------------------------------------------------------------------------------------------------
// The lane body.  src[p]: plane p's byte of the block's element 0 (a workspace region, a sub-slot or a stored plane); bsrc: the base's bytes
// of the block's element 0, xbase + (t.src + first) * W — 16-byte aligned, src being a multiple of 16 elements and the base 16-byte aligned;
// at: the output element of the block's element 0 (modulo 2^64: a head's may lie below 0); [lo, hi): the block's elements inside the range.
// A whole block: W 16-byte plane loads and, with a base, W 16-byte base loads, all before the first use; merge16, the XOR, and W 16-byte
// stores where the output address allows it, 16 element-wide stores otherwise.  The head and the tail of a range move element by element,
// byte by byte, and read base bytes of their own elements only: nothing outside the range is read from a stored plane or from the base —
// so nothing at or beyond elem_size * elements of a base — and nothing outside it is written.  With RuleNone `bsrc` is not looked at.
// ---------------------------------------------------------------------------------------------------------------
template <uint32_t W, typename Rule>
__device__ __forceinline__ void merge_block(const uint8_t *const (&src)[W], const uint8_t *__restrict__ bsrc, uint64_t at, uint32_t lo, uint32_t hi, uint8_t *__restrict__ out)
{
  static_assert(std::is_same<Rule, RuleNone>::value || std::is_same<Rule, RuleXor>::value, "the XOR is spelled out below: no other rule yet");
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], b[Rule::kBase ? 4 * W : 1], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
    if constexpr (Rule::kBase)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        load16(bsrc + 16 * k, b + 4 * k);
    }
    merge16<W>(pl, e);
    if constexpr (Rule::kBase)
    {
#pragma unroll
      for (uint32_t k = 0; k < 4 * W; k++)
        e[k] ^= b[k];
    }
    uint8_t *dst = out + at * W;
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
  for (uint32_t i = lo; i < hi; i++)
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
    {
      uint8_t b = 0;
      if constexpr (Rule::kBase)
        b = bsrc[i * W + p]; // (a base byte of the range's own element)
      out[(at + i) * W + p] = src[p][i] ^ b;
    }
}

// the lane's part of a task: elements [src + first, src + first + 16) cut to [lo, hi) of the task (t.lo < 16: only lane 0 has a head);
// false: the lane's block lies beyond the task
struct Block
{
  uint32_t first, lo, hi;
};
__device__ __forceinline__ bool block_of(uint32_t t_lo, uint32_t t_hi, Block *b)
{
  b->first = threadIdx.x * kLaneElements;
  if (b->first >= t_hi)
    return false;
  b->lo = b->first < t_lo ? t_lo - b->first : 0;
  b->hi = t_hi - b->first < kLaneElements ? t_hi - b->first : kLaneElements;
  return true;
}

// ---- one frame, ranges in device memory: k_planes_merge_indirect's task finding, planes.p[p] the workspace region where bit p of
// work_mask is set, else the stored plane ----
template <uint32_t W>
__device__ __forceinline__ void merge_task_single(const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask t, const uint8_t *__restrict__ xbase,
                                                  uint8_t *__restrict__ out)
{
  Block b;
  if (!block_of(t.lo, t.hi, &b))
    return;
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    src[p] = planes.p[p] + (((work_mask >> p) & 1) != 0 ? t.work_pos : t.src) + b.first;
  merge_block<W, RuleXor>(src, xbase + (t.src + b.first) * W, t.src + b.first + (uint64_t)t.dst_delta, b.lo, b.hi, out);
}

// Any grid: workgroup g serves tasks g, g + grid, ... below the total the cut left (k_planes_merge_indirect's walk)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_indirect_delta(PlanePtrs planes, uint32_t work_mask, const PlanesRange *__restrict__ ranges,
                                                                          const uint32_t *__restrict__ header, const uint32_t *__restrict__ first_task,
                                                                          const uint64_t *__restrict__ bases, const uint8_t *__restrict__ xbase, uint8_t *__restrict__ out)
{
  const uint32_t total = uni(header[kPlanesWsTotal]);
  if (blockIdx.x >= total)
    return;
  const uint32_t n = uni(header[kPlanesWsCount]);
  for (uint32_t t = blockIdx.x; t < total; t += gridDim.x)
  {
    const uint32_t r = task_row(first_task, n, t);
    const uint64_t offset = uni64(ranges[r].offset), length = uni64(ranges[r].length), dst_offset = uni64(ranges[r].dst_offset);
    const PlanesGatherTask task = planes_task_at<PlanesGatherTask>(offset, length, dst_offset, uni64(bases[r]), t - uni(first_task[r]));
    merge_task_single<W>(planes, work_mask, task, xbase, out);
  }
}

// ---- rows of many frames: the task as the workgroup holds it (every field the same on every lane) and its member's record, as the plain
// batch merges read them; xbase: the member's base, 0 (never looked at) under RuleNone ----
struct Task
{
  uint64_t src, work_pos, plane_step, dst_delta;
  uint32_t lo, hi;
};

template <uint32_t W, typename Rule>
__device__ __forceinline__ void merge_task_member(const Task &t, const PlanesGatherBatchMember *m, uint64_t xbase, const uint8_t *work, uint8_t *__restrict__ out)
{
  Block b;
  if (!block_of(t.lo, t.hi, &b))
    return;
  const uint32_t coded_mask = uni(m->coded_mask);
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
  {
    const uint64_t stored = uni64((uint64_t)m->stored[p]); // (read whether used or not: W loads at once, not one behind each branch)
    const uint64_t at = ((coded_mask >> p) & 1) != 0 ? (uint64_t)work + t.work_pos + p * t.plane_step : stored + t.src;
    src[p] = global_at(at) + b.first;
  }
  const uint8_t *bsrc = Rule::kBase ? global_at(xbase) + (t.src + b.first) * W : nullptr;
  merge_block<W, Rule>(src, bsrc, t.src + b.first + t.dst_delta, b.lo, b.hi, out);
}

template <typename Rule>
__device__ __forceinline__ void merge_member(const Task &t, const PlanesGatherBatchMember *m, uint64_t xbase, const uint8_t *work, uint8_t *__restrict__ out)
{
  const uint32_t W = uni(m->W);
  if (W == 2)
    merge_task_member<2, Rule>(t, m, xbase, work, out);
  else if (W == 4)
    merge_task_member<4, Rule>(t, m, xbase, work, out);
  else if (W == 8)
    merge_task_member<8, Rule>(t, m, xbase, work, out);
}

// a member with a base takes the delta body, one without the plain one: a branch on a scalar, per workgroup (k_planes_merge_delta_batch's)
__device__ __forceinline__ void merge_with_base(const Task &t, const PlanesGatherBatchMember *members, const uint64_t *__restrict__ xbases, uint32_t member, const uint8_t *work,
                                                uint8_t *__restrict__ out)
{
  const uint64_t xbase = uni64(xbases[member]);
  if (xbase != 0)
    merge_member<RuleXor>(t, members + member, xbase, work, out);
  else
    merge_member<RuleNone>(t, members + member, 0, work, out);
}

// grid: one workgroup per task of the list
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges_batch_delta(const PlanesGatherBatchTask *__restrict__ tasks, const PlanesGatherBatchMember *__restrict__ members,
                                                                              const uint64_t *__restrict__ xbases, const uint8_t *work, uint8_t *__restrict__ out)
{
  const PlanesGatherBatchTask *task = tasks + blockIdx.x;
  Task t;
  t.src = uni64(task->src);
  t.work_pos = uni64(task->work_pos);
  t.plane_step = uni64(task->plane_step);
  t.dst_delta = uni64((uint64_t)task->dst_delta);
  t.lo = uni(task->lo);
  t.hi = uni(task->hi);
  merge_with_base(t, members, xbases, uni(task->member), work, out);
}

// Any grid: k_planes_merge_batch_indirect's walk (bases[]: the rows' C_r; xbases[]: the members' base tensors)
__global__ __launch_bounds__(kThreads) void k_planes_merge_batch_indirect_delta(const PlanesSetRow *__restrict__ ranges, const uint32_t *__restrict__ header,
                                                                                const uint32_t *__restrict__ first_task, const uint64_t *__restrict__ bases,
                                                                                const PlanesGatherBatchMember *__restrict__ members, const uint64_t *__restrict__ xbases,
                                                                                const uint8_t *work, uint8_t *__restrict__ out)
{
  const uint32_t total = uni(header[kPlanesWsTotal]);
  if (blockIdx.x >= total)
    return;
  const uint32_t n = uni(header[kPlanesWsCount]);
  for (uint32_t t = blockIdx.x; t < total; t += gridDim.x)
  {
    const uint32_t r = task_row(first_task, n, t);
    const PlanesSetRow *row = ranges + r;
    const uint64_t offset = uni64(row->offset), length = uni64(row->length), dst_offset = uni64(row->dst_offset);
    const PlanesGatherTask cut = planes_task_at<PlanesGatherTask>(offset, length, dst_offset, uni64(bases[r]), t - uni(first_task[r]));
    const Task task{cut.src, cut.work_pos, planes_range_slot(offset, length), (uint64_t)cut.dst_delta, cut.lo, cut.hi};
    merge_with_base(task, members, xbases, uni(row->member), work, out);
  }
}
} // namespace

// A workgroup is 4 waves, one per SIMD, so a CU holds as many workgroups as a SIMD holds waves of the kernel.  The delta bodies hold the
// base's dwords beside the elements' and the planes', so these are not the plain merges' figures: each is its kernel's line of the
// compiler's report (tests/test_planes_gather_delta_resources.py holds the report against them) — 51, 61 and 101 VGPRs for 2-, 4- and
// 8-byte elements (the plain k_planes_merge_indirect<8>: 68, 7 waves), 70 for the table-driven kernel, which serves every element size.
constexpr uint32_t kMergeIndirectDeltaWavesPerSimd2 = 8;
constexpr uint32_t kMergeIndirectDeltaWavesPerSimd4 = 8;
constexpr uint32_t kMergeIndirectDeltaWavesPerSimd8 = 4;
constexpr uint32_t kMergeBatchIndirectDeltaWavesPerSimd = 7;

uint32_t planes_merge_indirect_delta_grid(uint32_t num_cus, uint32_t W, uint32_t max_count, uint64_t stride)
{
  const uint64_t most = (uint64_t)max_count + stride / kPlanesGatherTaskElements;
  const uint32_t waves = W == 2 ? kMergeIndirectDeltaWavesPerSimd2 : W == 4 ? kMergeIndirectDeltaWavesPerSimd4 : kMergeIndirectDeltaWavesPerSimd8;
  const uint64_t resident = (uint64_t)std::max(1u, num_cus) * waves;
  return (uint32_t)std::max<uint64_t>(1, std::min(most, resident));
}

uint32_t planes_merge_batch_indirect_delta_grid(uint32_t num_cus, uint32_t min_W, uint32_t max_count, uint64_t work_bytes)
{
  const uint64_t most = (uint64_t)max_count + work_bytes / ((uint64_t)std::max(1u, min_W) * kPlanesGatherTaskElements);
  const uint64_t resident = (uint64_t)std::max(1u, num_cus) * kMergeBatchIndirectDeltaWavesPerSimd;
  return (uint32_t)std::max<uint64_t>(1, std::min(most, resident));
}

hipError_t launch_planes_merge_indirect_delta(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesRange *d_ranges, const uint32_t *d_header,
                                              const uint32_t *d_first_task, const uint64_t *d_base, const void *xbase, uint32_t grid, void *out, hipStream_t stream)
{
  if (!planes_ptrs_ok(W, planes) || out == nullptr || ((uintptr_t)out & 15) != 0 || d_ranges == nullptr || ((uintptr_t)d_ranges & 7) != 0 || d_header == nullptr ||
      d_first_task == nullptr || d_base == nullptr || grid == 0 || grid > 0x7FFFFFFFu || (work_mask >> W) != 0 || xbase == nullptr || ((uintptr_t)xbase & 15) != 0)
    return hipErrorInvalidValue;
  uint8_t *dst = (uint8_t *)out;
  const uint8_t *xb = (const uint8_t *)xbase;
  (void)hipGetLastError();
  planes_with_width(W, [&](auto w) { k_planes_merge_indirect_delta<w()><<<grid, kThreads, 0, stream>>>(planes, work_mask, d_ranges, d_header, d_first_task, d_base, xb, dst); });
  return hipGetLastError();
}

hipError_t launch_planes_merge_ranges_batch_delta(const PlanesGatherBatchTask *d_tasks, uint32_t n_tasks, const PlanesGatherBatchMember *d_members, const uint64_t *d_xbases,
                                                  const void *work, void *out, hipStream_t stream)
{
  if (d_tasks == nullptr || ((uintptr_t)d_tasks & 7) != 0 || d_members == nullptr || ((uintptr_t)d_members & 7) != 0 || n_tasks == 0 || n_tasks > 0x7FFFFFFFu ||
      work == nullptr || ((uintptr_t)work & 15) != 0 || out == nullptr || ((uintptr_t)out & 15) != 0 || d_xbases == nullptr || ((uintptr_t)d_xbases & 7) != 0)
    return hipErrorInvalidValue;
  k_planes_merge_ranges_batch_delta<<<n_tasks, kThreads, 0, stream>>>(d_tasks, d_members, d_xbases, (const uint8_t *)work, (uint8_t *)out);
  return hipGetLastError();
}

hipError_t launch_planes_merge_batch_indirect_delta(const PlanesSetRow *d_ranges, const uint32_t *d_header, const uint32_t *d_first_task, const uint64_t *d_base,
                                                    const PlanesGatherBatchMember *d_members, const uint64_t *d_xbases, const void *work, void *out, uint32_t grid,
                                                    hipStream_t stream)
{
  if (d_ranges == nullptr || ((uintptr_t)d_ranges & 7) != 0 || d_header == nullptr || d_first_task == nullptr || d_base == nullptr || d_members == nullptr ||
      ((uintptr_t)d_members & 7) != 0 || work == nullptr || ((uintptr_t)work & 15) != 0 || out == nullptr || ((uintptr_t)out & 15) != 0 || grid == 0 || grid > 0x7FFFFFFFu ||
      d_xbases == nullptr || ((uintptr_t)d_xbases & 7) != 0)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  k_planes_merge_batch_indirect_delta<<<grid, kThreads, 0, stream>>>(d_ranges, d_header, d_first_task, d_base, d_members, d_xbases, (const uint8_t *)work, (uint8_t *)out);
  return hipGetLastError();
}

} // namespace hsrans
