// hsrans_planes_gather.hip — k_planes_merge_ranges<W>: the interleave of hsrans_planes.hip for element RANGES of a frame
// (hsrans_decode_device_planes_gather).  One workgroup serves one task — at most 4096 elements of one range, cut on the source's 16-element
// grid (hsrans_planes_gather_tasks) — and a lane one aligned 16-element block of it.  A plane is read either from the call's workspace, where
// the gather put the coded planes' bytes (at the task's work_pos), or straight from the frame, where a stored plane lies (at the task's
// src): both keep the source's alignment, so a whole block is one aligned 16-byte load per plane.  A whole block goes through merge16 and
// leaves as W 16-byte stores where its output address allows it, as 16 element-wide stores otherwise (dst_offset is in elements: the
// address is always a multiple of W); the head and the tail of a range are moved element by element, byte by byte, so that nothing
// outside the range is read from a stored plane or written to the output.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

namespace hsrans
{
namespace
{
using namespace planes_detail;

static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements, "one lane per 16-element block of a task");

// grid: one workgroup per task; work_mask bit p: planes.p[p] is a workspace region (indexed by work_pos), else a stored plane (indexed by src)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges(PlanePtrs planes, uint32_t work_mask, const PlanesGatherTask *__restrict__ tasks, uint8_t *__restrict__ out)
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
} // namespace

hipError_t launch_planes_merge_ranges(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks, const void *base,
                                      PlanesRule rule, void *out, hipStream_t stream)
{
  if (!planes_ptrs_ok(W, planes) || out == nullptr || ((uintptr_t)out & 15) != 0 || ((uintptr_t)base & 15) != 0 || d_tasks == nullptr ||
      ((uintptr_t)d_tasks & 7) != 0 || n_tasks == 0 || n_tasks > 0x7FFFFFFFu || (work_mask >> W) != 0)
    return hipErrorInvalidValue;
  uint8_t *dst = (uint8_t *)out;
  if (base != nullptr)
    planes_base_merge_ranges_kernel(rule, W, planes, work_mask, d_tasks, n_tasks, (const uint8_t *)base, dst, stream);
  else
    planes_with_width(W, [&](auto w) { k_planes_merge_ranges<w()><<<n_tasks, kThreads, 0, stream>>>(planes, work_mask, d_tasks, dst); });
  return hipGetLastError();
}

} // namespace hsrans
