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

// grid: one lane per 16 whole elements (at least one workgroup); n: elements
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_split(const uint8_t *__restrict__ in, uint64_t n, PlanePtrs planes)
{
  const uint64_t whole = n / kLaneElements, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (lane < whole)
  {
    uint32_t e[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(in + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
    split16<W>(e, pl);
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      store16(planes.p[p] + lane * kLaneElements, pl[p]);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      planes.p[p][i] = in[i * W + p];
  }
}

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

bool launch_ok(uint32_t W, const void *elements, uint64_t n, const PlanePtrs &planes)
{
  return planes_ptrs_ok(W, planes) && elements != nullptr && ((uintptr_t)elements & 15) == 0 && n != 0 && n <= kPlanesMaxElements;
}
uint32_t grid_of(uint64_t n)
{
  const uint64_t whole = n / kLaneElements;
  return (uint32_t)std::max<uint64_t>((whole + kThreads - 1) / kThreads, 1);
}
} // namespace

hipError_t launch_planes_split(uint32_t W, const void *in, uint64_t n, const PlanePtrs &planes, hipStream_t stream)
{
  if (!launch_ok(W, in, n, planes))
    return hipErrorInvalidValue;
  const uint8_t *src = (const uint8_t *)in;
  if (W == 2)
    k_planes_split<2><<<grid_of(n), kThreads, 0, stream>>>(src, n, planes);
  else if (W == 4)
    k_planes_split<4><<<grid_of(n), kThreads, 0, stream>>>(src, n, planes);
  else
    k_planes_split<8><<<grid_of(n), kThreads, 0, stream>>>(src, n, planes);
  return hipGetLastError();
}

hipError_t launch_planes_merge(uint32_t W, const PlanePtrs &planes, uint64_t n, void *out, hipStream_t stream)
{
  if (!launch_ok(W, out, n, planes))
    return hipErrorInvalidValue;
  uint8_t *dst = (uint8_t *)out;
  if (W == 2)
    k_planes_merge<2><<<grid_of(n), kThreads, 0, stream>>>(planes, n, dst);
  else if (W == 4)
    k_planes_merge<4><<<grid_of(n), kThreads, 0, stream>>>(planes, n, dst);
  else
    k_planes_merge<8><<<grid_of(n), kThreads, 0, stream>>>(planes, n, dst);
  return hipGetLastError();
}

} // namespace hsrans
