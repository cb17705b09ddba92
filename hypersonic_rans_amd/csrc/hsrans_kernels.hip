// gfx950 (MI355X, CDNA4) kernels for the hypersonic-rANS 32-bit-state / 16-bit-word decode path.
//
// What is computed (reference: /root/reference/src, scalar form rANS32x64_16w.cpp:223-250 = block_codec64.h:182-213):
//   for every group of S symbols, for state j = 0..S-1 in order:
//       slot = x_j & (2^bits - 1);  sym = cumulInv[slot];  out[i + idx2idx[j]] = sym;
//       x_j  = (x_j >> bits) * freq[sym] + slot - cumul[sym];
//       if (x_j < 2^15) x_j = (x_j << 16) | *readHead++;
//
// How it is mapped to a wave64 (one wavefront = one chain of the decode plan, hsrans_plan.h):
//   * lane j owns state j.  All S table steps happen at once; the only cross-lane dependency is the read cursor:
//     `readHead++` in ascending j  ==  lane j reads word[cur + popcount(renorm_mask & lanes_below_j)], i.e.
//     v_cmp -> SGPR-pair mask, v_mbcnt_lo/hi for the lane's rank, s_bcnt1 to advance the (scalar) cursor.
//   * decode table lives in LDS.  bits <= 12: one uint32 per slot = sym | (freq-1) << 8 | (slot-cumul) << 20
//     (freq-1 so that freq == 4096 fits — the reference's own packed table cannot, hist.cpp:304).
//     bits >= 13: uint8 sym[2^bits] + uint32 {freq | cumul << 16}[256] (two dependent LDS reads, as the reference's
//     hist_dec2_t path, hist.h:42-47).  The table is built in-kernel from the 256 uint16 counts in the stream.
//   * the uint16 stream is staged through a 2 KiB LDS ring per wave, refilled 1 KiB at a time by one coalesced,
//     bounds-checked buffer_load_dwordx4 per lane that is issued ~25 groups before it is needed.
//   * idx2idx maps 4 consecutive lanes to 4 consecutive output bytes (it is the bit permutation
//     j -> (j&0x23)|((j&4)<<2)|((j&0x18)>>1)), so a quad assembles one output dword with two DPP quad_perm ORs;
//     four groups are accumulated so that every lane stores one dword and the wave writes 4*S contiguous bytes.
//   * no MFMA: this is integer gather work; the roofline that bounds it is HBM (compressed bytes in + decoded bytes out).
//
// ONE device translation unit, in parts by kernel family (included below in dependency order):
//   kernels_layout.h    ring sizes, table layouts (kMode*), LDS layout, wave classes: what the kernels share with the host's launch policy
//   kernels_common.h    ring, table build, group step + hand-scheduled groups, output path, generic chain runner
//   kernels_persist.h   k_decode_persist   uniform-interval raw plans (static runs + ticket queues)
//   kernels_direct.h    k_decode_direct    one chain (run of chains) per wave: the headline; k_calibrate
//   kernels_batch.h     k_decode_batch     K independent streams in one launch of the one-chain-per-wave form
//   kernels_grouped.h   k_decode_grouped   block_/mt_ plans with checkpoints (BASELINE config 4)
//   kernels_spread.h    k_decode_spread    the same plans with few, large blocks: the chains dealt out evenly, two tables per workgroup
//   kernels_dealt.h     k_decode_dealt     the same in one round with HOST-dealt shares (<= 2 blocks each), two dependent trips before the first group
//   kernels_generic.h   k_decode           mt_ without index, block_ header walk, index-build passes
//   kernels_dual.h      k_decode_dual      two chains per wave (13-15 bits)
//   kernels_single.h    k_decode_single    one dependent chain (raw stream without index)
//   kernels_walk.h      k_mt_chase / k_mt_fill   K2: the mt_ header chain on the device; k_index_count / k_index_fill, k_walk_index_count / k_walk_index_fill   the indexed plan behind a first decode (mt_, block_)
//   kernels_gather.h    k_gather           byte ranges of one stream: one wave per task, entered at the chain that holds its first byte
//   kernels_index_batch.h   k_index_pass_batch   the first decode of many streams: one wavefront per walk / mt_ block; k_index_count_batch ... k_walk_index_fill_batch   their plans behind it
//                       k_gather_cut, k_gather_ranges   the same for ranges in device memory: checked and counted on the device, waves stride over the tasks; k_gather_set   byte ranges of many streams: every task names its member, one launch per table layout; k_set_cut, k_set_ranges   the same for ranges in device memory
// This file: the kernels and what names them — the kernel tables, prepare_kernels, launch_decode and the other launch_* functions.
// What decides a launch (table choice, launch shapes, choose_launch, shares and class weights, hsrans_index_boundaries' chain lengths) is
// host arithmetic in a unit of its own, hsrans_launch.cpp (hsrans_launch.h), which includes none of the kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hsrans_kernels.h"
#include "hsrans_plan.h"

#include "kernels_common.h"
#include "kernels_persist.h"
#include "kernels_direct.h"
#include "kernels_grouped.h"
#include "kernels_spread.h"
#include "kernels_dealt.h"
#include "kernels_generic.h"
#include "kernels_dual.h"
#include "kernels_batch.h"
#include "kernels_single.h"
#include "kernels_walk.h"
#include "kernels_gather.h"
#include "kernels_index_batch.h"

#include <algorithm>
#include <array>
#include <type_traits>
#include <vector>

namespace hsrans
{

hipError_t launch_mt_chase(const uint8_t *d_stream, uint64_t stream_len, uint64_t out_cap, uint32_t S, uint64_t *d_blocks, uint32_t max_blocks, WalkResult *d_result,
                           hipStream_t stream)
{
  (void)hipGetLastError(); // (the runtime's last error is sticky per thread: an earlier failed call must not be reported as this launch's)
  hipLaunchKernelGGL(k_mt_chase, dim3(1), dim3(64), 0, stream, d_stream, stream_len, out_cap, S, d_blocks, max_blocks, d_result);
  return hipGetLastError();
}

hipError_t launch_index_assemble(const IndexArgs &a, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_index_count, dim3(1), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(k_index_fill, dim3(a.n_base), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_index_assemble_walk(const WalkIndexArgs &a, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_walk_index_count, dim3(1), dim3(1024), 0, stream, a);
  // (the block count is on the device: wavefronts stride over the blocks there are, or leave)
  hipLaunchKernelGGL(k_walk_index_fill, dim3(a.max_blocks < 2048 ? (a.max_blocks ? a.max_blocks : 1) : 2048), dim3(64), 0, stream, a);
  return hipGetLastError();
}

// ---- hsrans_decode_device_indexing_batch's launches: at most kIndexPassModes of the pass, one count and one fill per kind ----
static const void *const g_index_pass_kernels[kIndexPassModes] = {(const void *)k_index_pass_batch<kModePack>, (const void *)k_index_pass_batch<kModePackM1>,
                                                                  (const void *)k_index_pass_batch<kModeTwoLevel>};

hipError_t launch_index_pass_batch(int mode, uint32_t max_bits, const IndexPassTask *d_tasks, uint32_t n_tasks, const IndexPassMember *d_members, hipStream_t stream)
{
  if (mode != index_pass_mode(max_bits) || max_bits > 15 || n_tasks == 0 || n_tasks > 0x7FFFFFFFu)
    return hipErrorInvalidValue;
  const uint32_t lds = kWaveRingBytes + ((table_bytes_for(mode, max_bits) + 15) & ~15u); // one wave: ring, then table
  (void)hipGetLastError();
  if (mode == kModePack)
    hipLaunchKernelGGL(k_index_pass_batch<kModePack>, dim3(n_tasks), dim3(64), lds, stream, d_tasks, d_members);
  else if (mode == kModePackM1)
    hipLaunchKernelGGL(k_index_pass_batch<kModePackM1>, dim3(n_tasks), dim3(64), lds, stream, d_tasks, d_members);
  else
    hipLaunchKernelGGL(k_index_pass_batch<kModeTwoLevel>, dim3(n_tasks), dim3(64), lds, stream, d_tasks, d_members);
  return hipGetLastError();
}

hipError_t launch_index_assemble_batch(const IndexArgs *d_args, uint32_t n, uint32_t most_blocks, const uint32_t *const *d_status_of, uint32_t *d_status_out, hipStream_t stream)
{
  if (n == 0 || n > 65536)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_index_count_batch, dim3(n), dim3(1024), 0, stream, d_args, d_status_of, d_status_out);
  hipLaunchKernelGGL(k_index_fill_batch, dim3(n, index_fill_rows(n, most_blocks)), dim3(64), 0, stream, d_args);
  return hipGetLastError();
}

hipError_t launch_index_assemble_walk_batch(const WalkIndexArgs *d_args, uint32_t n, uint32_t most_blocks, const uint32_t *const *d_status_of, uint32_t *d_status_out,
                                            hipStream_t stream)
{
  if (n == 0 || n > 65536)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_walk_index_count_batch, dim3(n), dim3(1024), 0, stream, d_args, d_status_of, d_status_out);
  hipLaunchKernelGGL(k_walk_index_fill_batch, dim3(n, index_fill_rows(n, most_blocks)), dim3(64), 0, stream, d_args);
  return hipGetLastError();
}

hipError_t launch_stream_checksum(const uint8_t *d_stream, uint64_t stream_len, uint64_t *d_sum, hipStream_t stream)
{
  hipError_t e = hipMemsetAsync(d_sum, 0, 8, stream);
  if (e != hipSuccess)
    return e;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_stream_checksum, dim3(kChecksumGrid), dim3(kChecksumBlock), 0, stream, d_stream, stream_len, (unsigned long long *)d_sum);
  return hipGetLastError();
}

hipError_t launch_mt_fill(const uint8_t *d_stream, uint64_t stream_len, uint32_t S, uint32_t bits, const uint64_t *d_blocks, uint8_t *d_plan, uint32_t n_chains,
                          uint64_t out_len, WalkResult *d_result, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_mt_fill, dim3(n_chains), dim3(64), 0, stream, d_stream, stream_len, S, bits, d_blocks, d_plan, n_chains, out_len, d_result);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// host-side launcher
// ---------------------------------------------------------------------------------------------------------------
// The kernel table: every instantiation a single-plan decode launch can run (KernelId), its name as a kernel trace prints it, and its launch.
// choose_launch picks the row, prepare_kernels raises every row's LDS limit, launch_decode launches through it: the one launch site.
struct KernelEntry
{
  const char *name;
  const void *fn;
  void (*launch)(const LaunchChoice &c, hipStream_t stream, const KParams &kp, const DealtParams &dp, const DealtTable *dt);
};
template <auto K>
static void launch_thunk(const LaunchChoice &c, hipStream_t stream, const KParams &kp, const DealtParams &dp, const DealtTable *dt)
{
  const auto go = [&](const auto &...args) { hipLaunchKernelGGL(K, dim3(c.grid), dim3(c.waves * 64), c.lds, stream, args...); };
  if constexpr (std::is_invocable_v<decltype(K), KParams>)
    go(kp);
  else
    go(dp, *dt); // (k_decode_dealt*: its own parameters + the dealing)
}
template <auto K>
static KernelEntry entry(const char *name)
{
  return {name, (const void *)K, launch_thunk<K>};
}
static const std::array<KernelEntry, kKernelCount> g_kernels = [] {
  std::array<KernelEntry, kKernelCount> t{};
  // (rows in the order the kernels have always been instantiated, which is the order of the compiler's resource report, build/hsrans_kernels.remarks)
  t[kKCalibrate] = entry<k_calibrate>("hsrans::k_calibrate");
  t[kKSingle] = entry<k_decode_single>("hsrans::k_decode_single");
  t[kKDecodePrivate + kModePack] = entry<k_decode<kModePack, false>>("hsrans::k_decode<0, false>");
  t[kKDecodeShared + kModePack] = entry<k_decode<kModePack, true>>("hsrans::k_decode<0, true>");
  t[kKDecodePrivate + kModePackM1] = entry<k_decode<kModePackM1, false>>("hsrans::k_decode<1, false>");
  t[kKDecodeShared + kModePackM1] = entry<k_decode<kModePackM1, true>>("hsrans::k_decode<1, true>");
  t[kKDecodePrivate + kModeTwoLevel] = entry<k_decode<kModeTwoLevel, false>>("hsrans::k_decode<2, false>");
  t[kKDecodeShared + kModeTwoLevel] = entry<k_decode<kModeTwoLevel, true>>("hsrans::k_decode<2, true>");
  t[kKDecodeShared + kModeRank] = entry<k_decode<kModeRank, true>>("hsrans::k_decode<4, true>");
  t[kKDecodeShared + kModeSpill] = entry<k_decode<kModeSpill, true>>("hsrans::k_decode<5, true>");
  t[kKDecodeShared + kModePack64] = entry<k_decode<kModePack64, true>>("hsrans::k_decode<3, true>");
  t[kKPersist] = entry<k_decode_persist<kModePack64>>("hsrans::k_decode_persist<3>");
  t[kKPersist + 1] = entry<k_decode_persist<kModeRank>>("hsrans::k_decode_persist<4>");
  t[kKDual] = entry<k_decode_dual<kModePack64>>("hsrans::k_decode_dual<3>");
  t[kKDual + 1] = entry<k_decode_dual<kModeRank>>("hsrans::k_decode_dual<4>");
  t[kKDirect + kModePack] = entry<k_decode_direct<kModePack>>("hsrans::k_decode_direct<0>");
  t[kKDirect + kModePackM1] = entry<k_decode_direct<kModePackM1>>("hsrans::k_decode_direct<1>");
  t[kKDirect + kModeTwoLevel] = entry<k_decode_direct<kModeTwoLevel>>("hsrans::k_decode_direct<2>");
  t[kKDirect + kModePack64] = entry<k_decode_direct<kModePack64>>("hsrans::k_decode_direct<3>");
  t[kKDirect + kModeRank] = entry<k_decode_direct<kModeRank>>("hsrans::k_decode_direct<4>");
  t[kKDirect + kModeSpill] = entry<k_decode_direct<kModeSpill>>("hsrans::k_decode_direct<5>");
  t[kKGrouped + kModePack] = entry<k_decode_grouped<kModePack, false>>("hsrans::k_decode_grouped<0, false, false>");
  t[kKGrouped + kModePackM1] = entry<k_decode_grouped<kModePackM1, false>>("hsrans::k_decode_grouped<1, false, false>");
  t[kKGrouped + kModeTwoLevel] = entry<k_decode_grouped<kModeTwoLevel, false>>("hsrans::k_decode_grouped<2, false, false>");
  t[kKGrouped + kModePack64] = entry<k_decode_grouped<kModePack64, false>>("hsrans::k_decode_grouped<3, false, false>");
  t[kKGroupedLean] = entry<k_decode_grouped<kModeTwoLevel, true>>("hsrans::k_decode_grouped<2, true, false>");
  t[kKGroupedLean + 1] = entry<k_decode_grouped<kModePack64, true>>("hsrans::k_decode_grouped<3, true, false>");
  t[kKGrouped + kModeRank] = entry<k_decode_grouped<kModeRank, false>>("hsrans::k_decode_grouped<4, false, false>");
  t[kKGroupedLean + 2] = entry<k_decode_grouped<kModeRank, true>>("hsrans::k_decode_grouped<4, true, false>");
  t[kKSpread] = entry<k_decode_spread<kModePack64>>("hsrans::k_decode_spread<3, false>");
  t[kKGroupedParts] = entry<k_decode_grouped<kModePack64, true, true>>("hsrans::k_decode_grouped<3, true, true>");
  t[kKGroupedParts + 1] = entry<k_decode_grouped<kModeRank, true, true>>("hsrans::k_decode_grouped<4, true, true>");
  t[kKSpread + 1] = entry<k_decode_spread<kModePack64, true>>("hsrans::k_decode_spread<3, true>");
  t[kKDealt] = entry<k_decode_dealt<true, false>>("hsrans::k_decode_dealt<true, false>");
  t[kKDealtNt] = entry<k_decode_dealt<false, false>>("hsrans::k_decode_dealt<false, false>");
  t[kKDealtParts] = entry<k_decode_dealt<true, true>>("hsrans::k_decode_dealt<true, true>");
  t[kKDealtRank] = entry<k_decode_dealt_rank<13, false>>("hsrans::k_decode_dealt_rank<13u, false>");
  t[kKDealtRank + 1] = entry<k_decode_dealt_rank<13, true>>("hsrans::k_decode_dealt_rank<13u, true>");
  t[kKDealtRank + 2] = entry<k_decode_dealt_rank<14, false>>("hsrans::k_decode_dealt_rank<14u, false>");
  t[kKDealtRank + 3] = entry<k_decode_dealt_rank<14, true>>("hsrans::k_decode_dealt_rank<14u, true>");
  return t;
}();
const char *kernel_name(KernelId k) { return g_kernels[k].name; }

// hsrans_decode_device_gather's kernels: a table per wave in the three layouts waves build for themselves, one table per workgroup in the
// three layouts the host builds (choose_table)
struct GatherKernel
{
  int mode;
  bool shared;
  const void *fn;
  void (*launch)(const GatherParams &gp, const GatherShape &shape, hipStream_t stream);
  const void *fn_ranges; // k_gather_ranges of the same table layout
  void (*launch_ranges)(const GatherParams &gp, const GatherRangesParams &rp, const GatherShape &shape, hipStream_t stream);
  const void *fn_set; // k_gather_set of the same table layout
  void (*launch_set)(const GatherSetParams &sp, const GatherShape &shape, hipStream_t stream);
  const void *fn_set_ranges; // k_set_ranges of the same table layout
  void (*launch_set_ranges)(const GatherSetRangesParams &rp, const GatherShape &shape, hipStream_t stream);
};
template <int MODE, bool SHARED>
static GatherKernel gather_entry()
{
  return {MODE, SHARED, (const void *)k_gather<MODE, SHARED>,
          [](const GatherParams &gp, const GatherShape &shape, hipStream_t stream) { hipLaunchKernelGGL((k_gather<MODE, SHARED>), dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, gp); },
          (const void *)k_gather_ranges<MODE, SHARED>,
          [](const GatherParams &gp, const GatherRangesParams &rp, const GatherShape &shape, hipStream_t stream) {
            hipLaunchKernelGGL((k_gather_ranges<MODE, SHARED>), dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, gp, rp);
          },
          (const void *)k_gather_set<MODE, SHARED>,
          [](const GatherSetParams &sp, const GatherShape &shape, hipStream_t stream) {
            hipLaunchKernelGGL((k_gather_set<MODE, SHARED>), dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, sp);
          },
          (const void *)k_set_ranges<MODE, SHARED>,
          [](const GatherSetRangesParams &rp, const GatherShape &shape, hipStream_t stream) {
            hipLaunchKernelGGL((k_set_ranges<MODE, SHARED>), dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, rp);
          }};
}
static const GatherKernel g_gather_kernels[] = {gather_entry<kModePack, false>(),  gather_entry<kModePackM1, false>(), gather_entry<kModeTwoLevel, false>(),
                                                gather_entry<kModePack64, true>(), gather_entry<kModeRank, true>(),    gather_entry<kModeSpill, true>()};

// per device (the CURRENT device): dynamic-LDS limit of every kernel variant, CU count
hipError_t prepare_kernels(DeviceGeom *geom)
{
  geom->max_lds = 160 * 1024;
  geom->num_cus = 256;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
    geom->num_cus = (uint32_t)cus;
  std::vector<const void *> fns;
  for (const KernelEntry &k : g_kernels)
    fns.push_back(k.fn);
  for (const void *fn : {(const void *)k_decode_batch<kModePack64>, (const void *)k_decode_grouped_batch<kModePack64>, (const void *)k_decode_batch_pair<kModePack64>,
                         (const void *)k_decode_batch_dual<kModePack64>, (const void *)k_decode_batch_dual<kModeRank>, (const void *)k_calibrate_batch})
    fns.push_back(fn);
  for (const void *fn : g_index_pass_kernels)
    fns.push_back(fn);
  for (const GatherKernel &g : g_gather_kernels)
  {
    fns.push_back(g.fn);
    fns.push_back(g.fn_ranges);
    fns.push_back(g.fn_set);
    fns.push_back(g.fn_set_ranges);
  }
  for (const void *fn : fns)
  {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)geom->max_lds);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

hipError_t launch_batch_direct(const BatchParams &bp, const BatchShape &shape, hipStream_t stream)
{
  (void)hipGetLastError();
  if (shape.kind == kBatchPair)
    hipLaunchKernelGGL(k_decode_batch_pair<kModePack64>, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  else if (shape.kind == kBatchDualPack)
    hipLaunchKernelGGL(k_decode_batch_dual<kModePack64>, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  else if (shape.kind == kBatchDualRank)
    hipLaunchKernelGGL(k_decode_batch_dual<kModeRank>, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  else if (bp.finish != nullptr)
    hipLaunchKernelGGL(k_calibrate_batch, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  else
    hipLaunchKernelGGL(k_decode_batch<kModePack64>, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  return hipGetLastError();
}

hipError_t launch_batch_grouped(const BatchGroupParams &bp, const BatchGroupShape &shape, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_decode_grouped_batch<kModePack64>, dim3(shape.grid), dim3(shape.waves * 64), shape.lds, stream, bp);
  return hipGetLastError();
}

// The targets of a sub-run launch: part k is complete once cum[k] + units[k] units have counted themselves into it, units[k] = the launch's
// units that overlap the part.  A unit of the spread and dealt launches is a workgroup's share of the chains, [share_begin(b),
// share_begin(b + 1)) for b < grid (the kernels count themselves by the same rule); grid == 0: the grouped launch, whose units are the plan's
// groups (PartPlan::group_units).
template <typename ShareBegin>
static void part_targets(const PartPlan &parts, uint32_t grid, ShareBegin share_begin, PartArgs *out, uint32_t units[kMaxLaunchParts])
{
  out->n = parts.n;
  uint32_t begin = 0;
  for (uint32_t k = 0; k < parts.n; k++)
  {
    const uint32_t end = parts.chain_end[k];
    units[k] = grid ? 0 : parts.group_units[k];
    for (uint32_t b = 0; b < grid && end > begin; b++)
    {
      const uint32_t c0 = share_begin(b), c1 = share_begin(b + 1);
      units[k] += c1 > c0 && c0 < end && c1 > begin ? 1 : 0;
    }
    out->chain_end[k] = end;
    out->target[k] = parts.cum[k] + units[k];
    begin = end > begin ? end : begin;
  }
}

hipError_t launch_decode(const Tuning &tn, const KParams &kp_in, const PlanHeader &h, const DeviceGeom &dg, hipStream_t stream, LaunchInfo *info, const PartPlan *parts, const DealtTable *dealt,
                         const uint32_t *dealt_weights)
{
  const LaunchChoice c = choose_launch(tn, h, dg, launch_facts(kp_in, parts, dealt != nullptr ? dealt_weights : nullptr));
  if (c.error != hipSuccess)
    return c.error;
  KParams kp = kp_in;
  DealtParams dp; // (k_decode_dealt's own parameters: filled for that launch only)
  uint32_t units[kMaxLaunchParts];
  if (c.spread == 2)
  {
    dp = DealtParams{};
    dp.stream = kp.stream;
    dp.stream_len = kp.stream_len;
    dp.stream_lo = kp.stream_lo;
    dp.out = kp.out;
    dp.out_cap = kp.out_cap;
    dp.pieces = (const Piece *)(kp.plan + plan_pieces_off(h.n_chains));
    dp.states = (const uint32_t *)(kp.plan + plan_states_off(h.n_chains, h.n_chains));
    dp.status = kp.status;
    dp.stamps = kp.stamps;
    dp.n_chains = h.n_chains;
    dp.bits = h.bits;
    memcpy(dp.cum, c.cum, sizeof(dp.cum));
    dp.gap_chains = c.gap_chains;
    if (parts != nullptr)
    {
      dp.parts = kp.parts;
      part_targets(*parts, c.grid, [&](uint32_t b) { return dealt->begin[b]; }, &dp.parts, units);
    }
  }
  else
  {
    kp.private_pair = c.shape.private_pair;
    if (kp.groups != nullptr && kp.ckpt_interval == 0 && kp.ckpt_groups == nullptr) // (grouped and spread launches)
      memcpy(kp.group_cum, c.cum, sizeof(kp.group_cum));
    if (kp.pa.pieces != nullptr && kp.pa.interval != 0)
    {
      kp.pa.static_per_wave = c.shares.static_per_wave;
      memcpy(kp.pa.run_len, c.shares.run_len, sizeof(kp.pa.run_len));
      memcpy(kp.pa.class_off, c.shares.class_off, sizeof(kp.pa.class_off));
      memcpy(kp.pa.wg_chains, c.shares.wg_chains, sizeof(kp.pa.wg_chains));
      memcpy(kp.pa.half_base, c.shares.half_base, sizeof(kp.pa.half_base));
      kp.pa.static_total = c.shares.static_total;
    }
    if (kp.pa.pieces != nullptr && kp.pa.interval == 0)
      kp.pa.run_chains = c.run_chains;
    if (c.spread == 1)
    {
      kp.pa.n_chains = h.n_chains; // (single-piece chains: n_pieces == n_chains)
      kp.pa.S = h.states;
      kp.pa.bits = h.bits;
    }
    if (parts != nullptr)
      part_targets(*parts, c.spread ? c.grid : 0, [&](uint32_t b) { return spread_share_begin(h.n_chains, b, c.grid, c.cum[0][c.waves], c.cum[1][c.waves]); }, &kp.parts, units);
  }
  if (info)
    *info = launch_info_of(c, h.n_chains);
  (void)hipGetLastError(); // (sticky per thread: an earlier failed call — e.g. an allocation a hostile stream asked for — is not this launch's error)
  g_kernels[c.kernel].launch(c, stream, kp, dp, dealt);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess && parts != nullptr) // (only now: a launch that was refused has counted nothing on the device)
    for (uint32_t k = 0; k < parts->n; k++)
      parts->cum[k] += units[k];
  return e;
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather's launches: functions of their own, beside choose_launch / launch_decode and touching neither
// (their shapes: gather_shape, gather_set_shape, gather_ranges_shape, gather_set_ranges_shape in hsrans_launch.cpp)
// ---------------------------------------------------------------------------------------------------------------
// the kernels of a launch shape; null with *why set where the shape cannot be launched (no grid, more LDS than a CU has) or names no table layout
static const GatherKernel *gather_kernel_for(const GatherShape &shape, hipError_t *why)
{
  *why = hipErrorInvalidValue;
  if (shape.grid == 0 || shape.lds > 160 * 1024)
    return nullptr;
  for (const GatherKernel &g : g_gather_kernels)
    if (g.mode == shape.mode && g.shared == shape.shared)
      return &g;
  *why = hipErrorNotSupported;
  return nullptr;
}

hipError_t launch_gather(const GatherParams &gp, const GatherShape &shape, hipStream_t stream)
{
  hipError_t e;
  const GatherKernel *g = gather_kernel_for(shape, &e);
  if (g == nullptr)
    return e;
  (void)hipGetLastError();
  g->launch(gp, shape, stream);
  return hipGetLastError();
}

// hsrans_decode_device_gather_batch's launch of one kind: k_gather_set of the kind's table layout
hipError_t launch_gather_set(const GatherSetParams &sp, const GatherShape &shape, hipStream_t stream)
{
  if (sp.n_tasks == 0 || (uint64_t)shape.grid * shape.waves < sp.n_tasks || (sp.table_bytes & 15) != 0)
    return hipErrorInvalidValue;
  hipError_t e;
  const GatherKernel *g = gather_kernel_for(shape, &e);
  if (g == nullptr)
    return e;
  (void)hipGetLastError();
  g->launch_set(sp, shape, stream);
  return hipGetLastError();
}

// hsrans_decode_device_gather_indirect's launches: k_gather_cut, then k_gather_ranges of the shape's table layout
hipError_t launch_gather_ranges(const GatherParams &gp, const GatherCutParams &cp, const GatherShape &shape, hipStream_t stream)
{
  if (cp.segment == 0)
    return hipErrorInvalidValue;
  hipError_t e;
  const GatherKernel *g = gather_kernel_for(shape, &e);
  if (g == nullptr)
    return e;
  GatherRangesParams rp{};
  rp.ranges = cp.ranges;
  rp.workspace = cp.workspace;
  rp.segment = cp.segment;
  rp.segment_shift = (cp.segment & (cp.segment - 1)) == 0 ? (uint32_t)__builtin_ctzll(cp.segment) : 0; // (a segment of 1 byte divides as it is)
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_gather_cut, dim3(1), dim3(1024), 0, stream, cp);
  e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  g->launch_ranges(gp, rp, shape, stream);
  return hipGetLastError();
}

// hsrans_decode_device_gather_batch_indirect's launches: k_set_cut, then k_set_ranges kind by kind
hipError_t launch_gather_set_ranges(const GatherSetCutParams &cp, uint8_t *dst, const GatherShape shapes[kGatherKinds], const uint32_t table_bytes[kGatherKinds], hipStream_t stream)
{
  const GatherKernel *kernels[kGatherKinds] = {};
  for (uint32_t k = 0; k < kGatherKinds; k++)
  {
    if (cp.kind_first[k] == cp.kind_first[k + 1])
      continue;
    hipError_t e;
    kernels[k] = gather_kernel_for(shapes[k], &e);
    if (kernels[k] == nullptr)
      return e;
    if (shapes[k].mode != (int)k || (table_bytes[k] & 15) != 0 || cp.kind_waves[k] != shapes[k].waves)
      return hipErrorInvalidValue;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_set_cut, dim3(1), dim3(1024), 0, stream, cp);
  hipError_t e = hipGetLastError();
  for (uint32_t k = 0; k < kGatherKinds && e == hipSuccess; k++)
  {
    if (kernels[k] == nullptr)
      continue;
    GatherSetRangesParams rp{};
    rp.ranges = cp.ranges;
    rp.workspace = cp.workspace;
    rp.members = cp.members;
    rp.dst = dst;
    rp.max_count = cp.max_count;
    rp.n_members = cp.n_members;
    rp.kind = k;
    rp.pos_lo = cp.kind_first[k];
    rp.pos_hi = cp.kind_first[k + 1];
    rp.table_bytes = table_bytes[k];
    kernels[k]->launch_set_ranges(rp, shapes[k], stream);
    e = hipGetLastError();
  }
  return e;
}

} // namespace hsrans
