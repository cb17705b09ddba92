// hsrans_planes.hip — k_planes_split<W> and k_planes_merge<W>: elements of W bytes (2, 4, 8) <-> W byte planes, plane[p][i] = elements[i * W + p].
// Pure streaming: the byte movement is the whole job.  A lane takes 16 consecutive elements — 16 W contiguous bytes of the element buffer
// (W 16-byte accesses) and 16 bytes of each plane (one 16-byte access per plane, consecutive lanes on consecutive 16 bytes) — and shuffles
// the bytes in registers with v_perm_b32 (a 4 x 4 byte transpose is 8 of them).  The last n % 16 elements are moved byte by byte, one
// element per lane, by the first lanes of the last workgroup.  (The shuffles themselves: planes_shuffle.h.)
#include "hsrans_planes.h"
#include "planes_shuffle.h"

#include <algorithm>

namespace hsrans
{
namespace
{
using namespace planes_detail;

// grid: one lane per 16 whole elements (at least one workgroup); n: elements.  (The lanes' work: split_lanes, planes_shuffle.h.)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_split(const uint8_t *__restrict__ in, uint64_t n, PlanePtrs planes)
{
  split_lanes<W, RuleNone>(in, nullptr, planes.p, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}

// merge_lanes<W, RuleNone> written out: as a call to it these three kernels read all their arguments on entry and came out 3 to 4 instructions
// shorter and SLOWER — on 128 MiB, medians of 48 over three rounds, 58.5 against 57.1 µs (W = 2), 66.8 against 66.2 (4), 75.0 against 74.0 (8),
// the first and the last beyond the quartiles of this form (CHANGELOG.md has the runs).  The splits lost nothing by the call.
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge(PlanePtrs planes, uint64_t n, uint8_t *__restrict__ out)
{
  const uint64_t whole = n / kLaneElements, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (lane < whole)
  {
    uint32_t e[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(planes.p[p] + lane * kLaneElements, pl[p]);
    merge16<W>(pl, e);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      store16(out + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      out[i * W + p] = planes.p[p][i];
  }
}

// the whole-tensor launchers' check, with or without a base
bool launch_ok(uint32_t W, const void *elements, const void *base, uint64_t n, const PlanePtrs &planes)
{
  return planes_ptrs_ok(W, planes) && elements != nullptr && ((uintptr_t)elements & 15) == 0 && ((uintptr_t)base & 15) == 0 && n != 0 && n <= kPlanesMaxElements;
}
uint32_t grid_of(uint64_t n)
{
  const uint64_t whole = n / kLaneElements;
  return (uint32_t)std::max<uint64_t>((whole + kThreads - 1) / kThreads, 1);
}
} // namespace

hipError_t launch_planes_split(uint32_t W, const void *in, const void *base, PlanesRule rule, uint64_t n, const PlanePtrs &planes, hipStream_t stream)
{
  if (!launch_ok(W, in, base, n, planes))
    return hipErrorInvalidValue;
  const uint8_t *src = (const uint8_t *)in;
  if (base != nullptr)
    planes_base_split_kernel(rule, W, grid_of(n), src, (const uint8_t *)base, n, planes, stream);
  else
    planes_with_width(W, [&](auto w) { k_planes_split<w()><<<grid_of(n), kThreads, 0, stream>>>(src, n, planes); });
  return hipGetLastError();
}

hipError_t launch_planes_merge(uint32_t W, const PlanePtrs &planes, const void *base, PlanesRule rule, uint64_t n, void *out, hipStream_t stream)
{
  if (!launch_ok(W, out, base, n, planes))
    return hipErrorInvalidValue;
  uint8_t *dst = (uint8_t *)out;
  if (base != nullptr)
    planes_base_merge_kernel(rule, W, grid_of(n), planes, (const uint8_t *)base, n, dst, stream);
  else
    planes_with_width(W, [&](auto w) { k_planes_merge<w()><<<grid_of(n), kThreads, 0, stream>>>(planes, n, dst); });
  return hipGetLastError();
}

} // namespace hsrans
