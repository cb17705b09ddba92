// kernels_layout.h — What the host's launch policy (hsrans_launch.cpp) and the decode kernels (kernels_common.h and the parts behind it) must
// agree on, and nothing else: the stream ring's sizes, the decode-table layouts, the LDS layout of a workgroup around one table, the wave
// classes.  Plain constants and constexpr functions: no device-only construct, so a host compiler builds it as it stands.
#ifndef HSRANS_KERNELS_LAYOUT_H
#define HSRANS_KERNELS_LAYOUT_H

#include <hip/hip_runtime.h> // (__host__ __device__: the header-only part)
#include <stdint.h>

namespace hsrans
{

constexpr uint32_t kRingSlots = 4;
constexpr uint32_t kChunkBytes = 512; // 32 lanes x 16 B
constexpr uint32_t kRingBytes = kRingSlots * kChunkBytes; // 2 KiB
// (the mirror is 128 bytes: the first 64 words of the ring, copied behind its end)
constexpr uint32_t kWaveRingBytes = kRingBytes + 256;     // per wave (ring + mirror, 256-byte granular)
// the hand-scheduled loop of k_decode_direct (run_groups_fast) keeps its read cursor as a plain LDS address that is only
// re-based every 4 groups, so it can run up to one chunk past the ring's end: the mirror there is a whole chunk
constexpr uint32_t kFastRingBytes = kRingBytes + kChunkBytes;
constexpr uint32_t kSingleMirror = 256;  // k_decode_single: ring entries mirrored behind the ring's end (4 groups x 64 words)

// decode-table layouts
constexpr int kModePack = 0;     // bits <= 11: uint32 per slot = sym | freq << 8 | (slot - cumul) << 20
constexpr int kModePackM1 = 1;   // bits == 12: same with freq - 1 (freq == 4096 must fit 12 bits)
constexpr int kModeTwoLevel = 2; // bits >= 13: uint8 sym[2^bits] + uint32 {freq | cumul << 16}[256]
constexpr int kModePack64 = 3;   // bits <= 14, table shared by a workgroup: uint2 per slot = {freq | sym << 24, slot - cumul}:
                                 // v_mad_u32_u24 takes freq (low 24 bits) and the bias operand as they are, v_perm takes byte 3

// bits >= 14 with a host-built table (persistent 64-state launches): uint8 rank[2^bits] — the slot's symbol as its RANK by
// frequency — followed by 256 x uint2 {freq | sym << 24, -cumul} ordered by rank.  A byte gather (the slot is the LDS address in
// k_decode_dual), then an 8-byte gather from a 2 KiB table in which the 32 most frequent symbols — nearly every lane of a group —
// sit in 32 different bank pairs; x' = freq * (x >> bits) + slot - cumul.  18 / 34 KiB at 14 / 15 bits instead of 128 / 256 KiB.
// (Round 2's layout for these widths was a coarse table of 4096 granules + a fine table for the granules that straddle a symbol
// boundary: 16.4 vector instructions and 11.2 LDS cycles per group against 12.3 and 13.3 here — 62.2 -> 56.7 us at 15 bits.)
constexpr int kModeRank = 4;
// The MODE 3 entries left in global memory ("spilled" table: L1/L2-resident, gathered with global_load_dwordx2): the
// comparison point BASELINE config 3 asks for next to the LDS-resident tables (HSRANS_TABLE_SPILL=1, host-built tables only)
constexpr int kModeSpill = 5;

__host__ __device__ constexpr uint32_t table_bytes_for(int mode, uint32_t bits)
{
  return mode == kModeSpill ? 0u
         : mode == kModeTwoLevel ? (1u << bits) + 1024
         : mode == kModePack64 ? 8u << bits
         : mode == kModeRank ? (1u << bits) + 2048u
                               : 4u << bits;
}

// Modes whose 64-state loop is hand-scheduled: their rings carry a whole-chunk mirror (kFastRingBytes per wave) ...
__host__ __device__ constexpr bool fast_ring_mode(int mode) { return mode == kModePack64 || mode == kModeRank; }
// ... and the one whose table sits at the START of the workgroup's LDS (address 0: the slot is the address of its rank byte)
__host__ __device__ constexpr bool table_first_mode(int mode) { return mode == kModeRank; }

// The LDS of a workgroup that shares ONE table, as byte offsets from its start: [waves x rings][table][extra], or with the table
// first [table][extra][waves x rings].  The launcher sizes the workgroup by total(), the kernels place their pointers by the rest
// (wave_ctx_lds), so the two cannot drift apart.
//   rings_per_wave: 2 in the dual kernels (one ring per chain)
//   extra: bytes behind the table; kGroupedExtra = run_grouped's two next-group words (64 B) and a table-build scratch of its own
//          (1 KiB, the last of them: a round's first stream chunks are requested before its table is built).  Without extra bytes
//          the build scratch is wave 0's ring: no request is in flight while a table is built
//   whole_mirror: every ring carries a whole-chunk mirror (the gather kernels never run the hand-scheduled loops: false)
//   table_given: the table's size where it is not worked out from mode and bits: a gather over many plans makes room for their largest
constexpr uint32_t kBuildScratchBytes = 1024; // counts + prefix sums, 512 B each
constexpr uint32_t kGroupedExtra = 64 + kBuildScratchBytes;
struct LdsLayout
{
  int mode;
  uint32_t bits, waves, rings_per_wave, extra;
  bool whole_mirror, given;
  uint32_t table_given;
  constexpr uint32_t table_bytes() const { return given ? table_given : table_bytes_for(mode, bits); }
  constexpr uint32_t ring_stride() const { return rings_per_wave * (whole_mirror ? kFastRingBytes : kWaveRingBytes); } // from one wave's rings to the next wave's
  constexpr uint32_t rings() const { return table_first_mode(mode) ? table_bytes() + extra : 0; }
  constexpr uint32_t table() const { return table_first_mode(mode) ? 0 : waves * ring_stride(); }
  constexpr uint32_t total() const { return waves * ring_stride() + table_bytes() + extra; }
};
__host__ __device__ constexpr LdsLayout lds_layout(int mode, uint32_t bits, uint32_t waves, uint32_t rings_per_wave = 1, uint32_t extra = 0)
{
  return LdsLayout{mode, bits, waves, rings_per_wave, extra, fast_ring_mode(mode), false, 0};
}
// (plain rings: the gather kernels never run the hand-scheduled loops)
__host__ __device__ constexpr LdsLayout lds_layout_gather(int mode, uint32_t table_bytes, uint32_t waves) { return LdsLayout{mode, 0, waves, 1, 0, false, true, table_bytes}; }

// The 8 wave classes every share rule weighs a wave by (the SIMD arbiter serves its oldest wave first, so equal shares finish far apart):
// class = (workgroup in the grid's second half ? 4 : 0) + wave in workgroup / (waves / 4), the fourth class taking what a workgroup of 12
// waves leaves over; workgroups of fewer than 4 waves have one wave per class.  The host's users are hsrans_launch.cpp, hsrans_batch_deal.cpp
// and hsrans_capi_calibrate.cpp; run_persistent and run_persistent_pair (kernels_persist.h) spell the same rule on the device.
constexpr uint32_t waves_per_class(uint32_t waves) { return waves >= 4 ? waves / 4 : 1; }
constexpr uint32_t wave_class(bool second_half, uint32_t wave_in_wg, uint32_t waves)
{
  return (second_half ? 4u : 0u) + (wave_in_wg / waves_per_class(waves) < 4 ? wave_in_wg / waves_per_class(waves) : 3u);
}

} // namespace hsrans

#endif // HSRANS_KERNELS_LAYOUT_H
