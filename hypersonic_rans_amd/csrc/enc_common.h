// enc_common.h — what every encoder kernel shares: constants, the coding wavefront's LDS, 2-byte-aligned word types, wave helpers.
// Part of the one encoder translation unit hsrans_encode.hip (which includes the parts in dependency order and holds the launchers).
#ifndef HSRANS_ENC_COMMON_H
#define HSRANS_ENC_COMMON_H

namespace hsrans
{
namespace
{

// Input bytes fetched per step of the rANS pass (CHUNK): the staging ring — two chunks — is most of a wavefront's LDS.  4 KiB chunks
// (13.25 KiB a wavefront, 11 wavefronts per CU) while every block of the launch is resident at once anyway: a block is then alone with
// its chain and pays for every chunk change; 2 KiB chunks (9.25 KiB, 17 per CU) beyond that: 100 MB in 32 KiB blocks 442 -> 501 GB/s
// (3,052 blocks: one round instead of two), 256 MiB 615 -> 685, 2^30 bytes 777 -> 822 GB/s; 100 MB in 64 KiB blocks lose 1 % with them.
constexpr uint32_t kChunkFew = 4096, kChunkMany = 2048;
constexpr uint32_t kSubHists = 8;        // histogram copies (lane & 7) of a wavefront that counts its own bytes, laid out [symbol][copy]
// The emitted words of the rANS pass go through an LDS ring and leave it in whole segments (one 8-byte store per lane) instead of
// one masked 2-byte global store per group: a group emits at most 128 bytes, a set of four groups at most one segment, so with a
// check after every set two segments are all the ring needs (byte o of the block's slot sits at ring offset o mod kOutRing)
constexpr uint32_t kOutSeg = 512;
constexpr uint32_t kOutRing = 2 * kOutSeg;

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }
__device__ __forceinline__ uint32_t enc_lane_to_byte(uint32_t j) { return (j & 0x23u) | ((j & 0x04u) << 2) | ((j & 0x18u) >> 1); }
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct __attribute__((packed, aligned(2))) U64a2
{
  uint64_t v;
};
struct __attribute__((packed, aligned(2))) U32a2
{
  uint32_t v;
};

template <uint32_t CHUNK>
struct WaveLdsT
{
  uint32_t order[256];      // count << 8 | symbol in heap-sort order; after the normalisation: the kOutRing bytes of the emitted-word ring
  uint4 table[256];         // {x_max, bias, rcp, cmpl | shift << 24}
  uint8_t stage[2 * CHUNK]; // the input ring (table and stage double as the kSubHists histogram copies before the table exists)
  uint32_t sink[64];        // where the lanes that emit nothing in a group put their write (a select of the address is cheaper than two writes of EXEC)
};
static_assert(sizeof(uint4) * 256 + 2 * kChunkMany >= kSubHists * 256 * 4, "histogram copies must fit");
static_assert(kOutRing == sizeof(uint32_t) * 256, "the emitted-word ring is the sort's order array");

__device__ __forceinline__ uint32_t ballot_count(bool pred) { return (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(pred)); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
  for (int d = 32; d >= 1; d >>= 1)
    v += __shfl_xor(v, d, 64);
  return __builtin_amdgcn_readfirstlane(v); // (every lane holds the total; said so, what is computed from it stays in scalar registers)
}

// inclusive prefix sum of `v` over the wavefront's lanes
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, uint32_t lane)
{
  for (int d = 1; d < 64; d <<= 1)
  {
    const T o = __shfl_up(v, d, 64);
    if ((int)lane >= d)
      v += o;
  }
  return v;
}

__device__ __forceinline__ uint4 load16_guarded(const uint8_t *in, uint64_t pos, uint64_t n)
{
  if (pos + 16 <= n)
    return *(const uint4 *)(in + pos);
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t k = 0; k < 16; k++)
    if (pos + k < n)
      w[k >> 2] |= (uint32_t)in[pos + k] << (8 * (k & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

} // namespace
} // namespace hsrans

#endif
