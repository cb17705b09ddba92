// hsrans_planes_gather_indirect.hip — hsrans_decode_device_planes_gather_indirect: the element ranges are in device memory and are read when
// the launches run.  k_planes_cut checks them, lays out their slots, counts their merge tasks and writes the rows of the set's gather;
// behind the set's own indirect call, k_planes_merge_indirect<W> interleaves the ranges: it finds each task's range in the prefix the cut
// left and derives the task by planes_task_at (planes_cut.h), the function the host's cut lists its tasks with.  Control workspace:
// PlanesCutWs (hsrans_planes.h).
// The merge's body is k_planes_merge_ranges' (hsrans_planes_gather.hip), restated here (planes_shuffle.h says why).
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
static_assert(sizeof(PlanesRange) == 24 && sizeof(PlanesSetRow) == 32, "the ranges' and the rows' ABI layout");

// ---------------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads: nothing is handed between workgroups inside the launch.  A round is kPlanesCutBatch consecutive ranges per
// thread, their loads issued together (a round is a chain of dependent loads; a range at a time it would pay the chain once per 1024
// ranges).  The slots (64-bit) and the task counts are scanned inside the wave by __shfl_up, over the 16 waves through LDS, with a carry
// from round to round (k_gather_cut's scan).  Every total a thread needs is in its registers — the carries are the same on every thread —
// so no word written here is read back here.  One range that fails planes_cut.h's rules, a count above max_count, a sum of slots above
// the regions' stride or 2^31 tasks or more refuses the whole call: task total and row count are written as 0 after the last round and
// kStatusBadRange is set.  Every word the set's launches and the merge read is written by every call.
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPlanesCutBatch = 2;

__global__ void __launch_bounds__(1024) k_planes_cut(PlanesCutParams cp)
{
  __shared__ uint64_t wave_slots[16], wave_tasks[16];
  __shared__ uint32_t any_bad;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t n = cp.count != nullptr ? *cp.count : cp.max_count;
  bool bad = n > cp.max_count;
  if (bad)
    n = 0;
  if (threadIdx.x == 0)
    any_bad = 0;
  __syncthreads();
  uint64_t slot_carry = 0, task_carry = 0; // of the rounds before this one (the same on every thread)
  for (uint64_t r0 = 0; r0 < n; r0 += 1024 * kPlanesCutBatch)
  {
    const uint64_t mine = r0 + (uint64_t)threadIdx.x * kPlanesCutBatch;
    PlanesRange g[kPlanesCutBatch];
    uint64_t slot[kPlanesCutBatch], tasks[kPlanesCutBatch], my_slots = 0, my_tasks = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatch; j++) // (no branch between the loads: rows beyond n read row 0 and do not count)
      g[j] = cp.ranges[mine + j < n ? mine + j : 0];
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatch; j++)
    {
      const bool in = mine + j < n;
      bool good = planes_source_ok(g[j].offset, g[j].length, cp.elements) && planes_dest_ok(g[j].dst_offset, g[j].length, cp.out_elements);
      slot[j] = good ? planes_range_slot(g[j].offset, g[j].length) : 0;
      good = good && slot[j] <= cp.stride; // (so that no sum below can wrap: stride <= 2^48, the entry's indirect_stride)
      if (!in || !good)
      {
        slot[j] = 0;
        g[j].length = 0;
      }
      tasks[j] = planes_range_tasks(g[j].offset, g[j].length);
      bad = bad || (in && !good);
      my_slots += slot[j];
      my_tasks += tasks[j];
    }
    // inclusive scans of the threads' sums: inside the wave, then over the 16 waves' sums
    uint64_t incl_slots = my_slots, incl_tasks = my_tasks;
    for (uint32_t d = 1; d < 64; d *= 2)
    {
      const uint64_t s = __shfl_up(incl_slots, d, 64), t = __shfl_up(incl_tasks, d, 64);
      if (lane >= d)
      {
        incl_slots += s;
        incl_tasks += t;
      }
    }
    __syncthreads(); // (the sums of the round before have been read)
    if (lane == 63)
    {
      wave_slots[wave] = incl_slots;
      wave_tasks[wave] = incl_tasks;
    }
    __syncthreads();
    uint64_t at = slot_carry, first = task_carry, round_slots = 0, round_tasks = 0;
    for (uint32_t w = 0; w < 16; w++)
    {
      const uint64_t s = wave_slots[w], t = wave_tasks[w];
      at += w < wave ? s : 0;
      first += w < wave ? t : 0;
      round_slots += s;
      round_tasks += t;
    }
    at += incl_slots - my_slots; // B_r of this thread's first range ...
    first += incl_tasks - my_tasks; // ... and its first task (a prefix at or above the limits is refused below: what is stored then is never read)
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatch; j++)
    {
      const uint64_t r = mine + j;
      if (r < n)
      {
        cp.first_task[r] = (uint32_t)first;
        cp.base[r] = at;
        const uint64_t phase = g[j].length != 0 ? (g[j].offset & 15) : 0;
#pragma unroll 1
        for (uint32_t k = 0; k < cp.coded; k++) // (a short loop kept rolled: unrolled by 4 ranges x 8 planes the stores spill)
          cp.rows[r * cp.coded + k] = PlanesSetRow{g[j].offset, g[j].length, (uint64_t)((cp.coded_planes >> (4 * k)) & 15) * cp.stride + at + phase, k, 0};
      }
      at += slot[j];
      first += tasks[j];
    }
    slot_carry += round_slots;
    task_carry += round_tasks;
    if (slot_carry > cp.stride)
    {
      bad = true;
      slot_carry = 0;
    }
    if (task_carry >= kPlanesCutLimit)
    {
      bad = true;
      task_carry = 0;
    }
  }
  if (bad)
    any_bad = 1; // (benign race: every writer stores 1)
  __syncthreads();
  if (threadIdx.x == 0)
  {
    const bool refuse = uni(any_bad) != 0; // (a scalar: it selects between the scalars n * coded and 0)
    cp.first_task[n] = (uint32_t)task_carry;
    cp.header[kPlanesWsTotal] = refuse ? 0 : (uint32_t)task_carry;
    cp.header[kPlanesWsCount] = n;
    cp.header[kPlanesWsRows] = refuse ? 0 : n * cp.coded;
    if (refuse)
      atomicOr(cp.status, kStatusBadRange);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The merge.  Any grid: workgroup b serves tasks b, b + grid, ... below the total the cut left; a workgroup whose first task lies beyond it
// returns.  A task's range is the last r with first_task[r] <= t (ranges without tasks share their successor's entry and are passed
// over), found by task_row (planes_shuffle.h); the task is planes_task_at's.
// ---------------------------------------------------------------------------------------------------------------

// this lane's aligned 16-element block of task t (k_planes_merge_ranges' body): a whole block is one aligned 16-byte load per plane, merge16
// and W 16-byte stores where its output address allows it, 16 element-wide stores otherwise; the head and the tail of a range move element
// by element, byte by byte, so that nothing outside the range is read from a stored plane or written to the output
template <uint32_t W>
__device__ __forceinline__ void merge_task(const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask t, uint8_t *__restrict__ out)
{
  const uint32_t first = threadIdx.x * kLaneElements; // the lane's block: elements [src + first, src + first + 16)
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements; // (t.lo < 16: only lane 0 has a head)
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    src[p] = planes.p[p] + (((work_mask >> p) & 1) != 0 ? t.work_pos : t.src) + first;
  const uint64_t base = t.src + first + (uint64_t)t.dst_delta; // the output element of the block's element 0 (modulo 2^64: a head's may lie below 0)
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
    merge16<W>(pl, e);
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
  for (uint32_t i = lo; i < hi; i++)
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      out[(base + i) * W + p] = src[p][i];
}

template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_indirect(PlanePtrs planes, uint32_t work_mask, const PlanesRange *__restrict__ ranges, const uint32_t *__restrict__ header,
                                                                    const uint32_t *__restrict__ first_task, const uint64_t *__restrict__ bases, uint8_t *__restrict__ out)
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
    merge_task<W>(planes, work_mask, task, out);
  }
}
} // namespace

// A workgroup is 4 waves, one per SIMD, so a CU holds as many workgroups as a SIMD holds waves of the kernel: 8 for 2- and 4-byte
// elements, 7 for 8-byte ones (68 VGPRs; tests/test_planes_gather_indirect_resources.py holds the compiler's report against these).
uint32_t planes_merge_indirect_grid(uint32_t num_cus, uint32_t W, uint32_t max_count, uint64_t stride)
{
  const uint64_t most = (uint64_t)max_count + stride / kPlanesGatherTaskElements;
  const uint64_t resident = (uint64_t)std::max(1u, num_cus) * (W == 8 ? 7 : 8);
  return (uint32_t)std::max<uint64_t>(1, std::min(most, resident));
}

hipError_t launch_planes_cut(const PlanesCutParams &cp, hipStream_t stream)
{
  if (cp.ranges == nullptr || cp.max_count == 0 || cp.coded > kPlanesMax || cp.header == nullptr || cp.first_task == nullptr || cp.base == nullptr || cp.rows == nullptr ||
      cp.status == nullptr)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_planes_cut, dim3(1), dim3(1024), 0, stream, cp);
  return hipGetLastError();
}

hipError_t launch_planes_merge_indirect(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesRange *d_ranges, const uint32_t *d_header,
                                        const uint32_t *d_first_task, const uint64_t *d_base, uint32_t grid, void *out, hipStream_t stream)
{
  if (!planes_ptrs_ok(W, planes) || out == nullptr || ((uintptr_t)out & 15) != 0 || d_ranges == nullptr || ((uintptr_t)d_ranges & 7) != 0 || d_header == nullptr ||
      d_first_task == nullptr || d_base == nullptr || grid == 0 || grid > 0x7FFFFFFFu || (work_mask >> W) != 0)
    return hipErrorInvalidValue;
  uint8_t *dst = (uint8_t *)out;
  (void)hipGetLastError();
  planes_with_width(W, [&](auto w) { k_planes_merge_indirect<w()><<<grid, kThreads, 0, stream>>>(planes, work_mask, d_ranges, d_header, d_first_task, d_base, dst); });
  return hipGetLastError();
}

} // namespace hsrans
