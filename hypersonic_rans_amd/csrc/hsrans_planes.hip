// hsrans_planes.hip — k_planes_split<W> and k_planes_merge<W>: elements of W bytes (2, 4, 8) <-> W byte planes, plane[p][i] = elements[i * W + p].
// Pure streaming: the byte movement is the whole job.  A lane takes 16 consecutive elements — 16 W contiguous bytes of the element buffer
// (W 16-byte accesses) and 16 bytes of each plane (one 16-byte access per plane, consecutive lanes on consecutive 16 bytes) — and shuffles
// the bytes in registers with v_perm_b32 (a 4 x 4 byte transpose is 8 of them).  The last n % 16 elements are moved byte by byte, one
// element per lane, by the first lanes of the last workgroup.
#include "hsrans_planes.h"

#include <algorithm>

namespace hsrans
{
namespace
{
constexpr uint32_t kThreads = 256;
constexpr uint32_t kLaneElements = 16;

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
  if ((W != 2 && W != 4 && W != 8) || elements == nullptr || ((uintptr_t)elements & 15) != 0 || n == 0 || n > kPlanesMaxElements)
    return false;
  for (uint32_t p = 0; p < W; p++)
    if (planes.p[p] == nullptr || ((uintptr_t)planes.p[p] & 15) != 0)
      return false;
  return true;
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
