// planes_shuffle.h — the in-register byte shuffles of the byte-plane kernels (hsrans_planes.hip, hsrans_planes_gather.hip): 16 elements of W
// bytes as they lie in memory <-> 16 bytes of each of the W planes, with v_perm_b32 (a 4 x 4 byte transpose is 8 of them).  Device code only;
// every function is inlined into the kernel that calls it.  Everything is in hsrans::planes_detail; the two units say `using namespace`.
#ifndef HSRANS_PLANES_SHUFFLE_H
#define HSRANS_PLANES_SHUFFLE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsrans
{
namespace planes_detail
{
inline constexpr uint32_t kThreads = 256;     // lanes of a workgroup of every byte-plane kernel
inline constexpr uint32_t kLaneElements = 16; // elements a lane moves

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
} // namespace planes_detail
} // namespace hsrans

#endif // HSRANS_PLANES_SHUFFLE_H
