// hsrans_planes_gather_batch.hip — k_planes_merge_ranges_batch: the interleave of element ranges (hsrans_planes_gather.hip) for rows of MANY
// frames in ONE launch (hsrans_decode_device_planes_gather_batch).  One workgroup serves one task — at most 4096 elements of one row, cut on
// the source's 16-element grid (hsrans_planes_gather_batch_tasks) — and reads, the same on every lane and on scalar loads, its 48-byte task
// and then the record of the task's member: the element size W, which planes were coded and where the stored planes lie.  It branches once
// on W into the body of k_planes_merge_ranges<W>, of which this unit has its own copy (one of five; planes_shuffle.h's note on what is NOT shared says why): a lane per aligned
// 16-element block, each plane one 16-byte load — a coded plane from the call's workspace (work_pos + p * plane_step: the row's sub-slot of plane p), a stored plane straight
// from its frame (the record's address + src) —, merge16, and W 16-byte stores where the output address allows it, element-wide stores
// otherwise; heads and tails move byte by byte, so nothing outside a range is read from a stored plane or written.  2-, 4- and 8-byte
// members share the launch.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

namespace hsrans
{
namespace
{
using namespace planes_detail;

static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements, "one lane per 16-element block of a task");
static_assert(sizeof(PlanesGatherBatchTask) == 48 && sizeof(PlanesGatherBatchMember) == 72, "the task list's and the member table's layout");

// the task as the workgroup holds it: every field the same on every lane
struct Task
{
  uint64_t src, work_pos, plane_step, dst_delta;
  uint32_t lo, hi;
};

// k_planes_merge_ranges<W>'s body for one task of a member of W-byte elements
template <uint32_t W>
__device__ __forceinline__ void merge_task(const Task &t, const PlanesGatherBatchMember *m, const uint8_t *work, uint8_t *__restrict__ out)
{
  const uint32_t first = threadIdx.x * kLaneElements; // the lane's block: elements [src + first, src + first + 16)
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements; // (t.lo < 16: only lane 0 has a head)
  const uint32_t coded_mask = uni(m->coded_mask);
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
  {
    const uint64_t stored = uni64((uint64_t)m->stored[p]); // (read whether used or not: W loads at once, not one behind each branch)
    const uint64_t at = ((coded_mask >> p) & 1) != 0 ? (uint64_t)work + t.work_pos + p * t.plane_step : stored + t.src;
    src[p] = global_at(at) + first;
  }
  const uint64_t base = t.src + first + t.dst_delta; // the output element of the block's element 0 (modulo 2^64: a head's may lie below 0)
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

// grid: one workgroup per task
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges_batch(const PlanesGatherBatchTask *__restrict__ tasks, const PlanesGatherBatchMember *__restrict__ members,
                                                                        const uint8_t *work, uint8_t *__restrict__ out)
{
  const PlanesGatherBatchTask *task = tasks + blockIdx.x;
  Task t;
  t.src = uni64(task->src);
  t.work_pos = uni64(task->work_pos);
  t.plane_step = uni64(task->plane_step);
  t.dst_delta = uni64((uint64_t)task->dst_delta);
  t.lo = uni(task->lo);
  t.hi = uni(task->hi);
  const PlanesGatherBatchMember *m = members + uni(task->member);
  const uint32_t W = uni(m->W);
  if (W == 2)
    merge_task<2>(t, m, work, out);
  else if (W == 4)
    merge_task<4>(t, m, work, out);
  else if (W == 8)
    merge_task<8>(t, m, work, out);
}
} // namespace

hipError_t launch_planes_merge_ranges_batch(const PlanesGatherBatchTask *d_tasks, uint32_t n_tasks, const PlanesGatherBatchMember *d_members, const void *work, void *out,
                                            hipStream_t stream)
{
  if (d_tasks == nullptr || ((uintptr_t)d_tasks & 7) != 0 || d_members == nullptr || ((uintptr_t)d_members & 7) != 0 || n_tasks == 0 || n_tasks > 0x7FFFFFFFu ||
      work == nullptr || ((uintptr_t)work & 15) != 0 || out == nullptr || ((uintptr_t)out & 15) != 0)
    return hipErrorInvalidValue;
  k_planes_merge_ranges_batch<<<n_tasks, kThreads, 0, stream>>>(d_tasks, d_members, (const uint8_t *)work, (uint8_t *)out);
  return hipGetLastError();
}

} // namespace hsrans
