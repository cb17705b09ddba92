// The gfx950 encoders (include/hsrans_hip.h: hsrans_encode_device, _raw, _ex, _batch, _ex_batch, hsrans_encode_host_pipelined): this file holds the
// launchers; the device code is in the enc_*.h parts included below, in dependency order:
//   enc_common.h     constants, the coding wavefront's LDS (WaveLdsT), 2-byte-aligned word types, lane / wave helpers, scans and sums
//   enc_normalise.h  the reference's count normalisation on one wavefront: the heap sort replayed in registers, adjust_counts
//   enc_pass.h       encode_body — one wavefront codes one block or one stream — and its stages; k_encode_blocks, k_encode_raw
//   enc_place.h      histograms, unit summaries and costs, scan, plan, gather and copy; k_encode_chain, k_gather_chain
//   enc_batch.h      the _batch kernels
//
// Every encode runs through encode_body: normalisation identical to hist.cpp:16-215 (the heap sort's extractions as straight-line scalar
// code) -> backward rANS pass, lane j = coder state j, a set of four groups as one asm statement, words through an LDS ring into a scratch
// slot top-down, then the header in front of them: the slot ends with the image.  Written for its INSTRUCTION COUNT: a wavefront alone on
// its SIMD pays about 2.3 ns per instruction, whatever it is (tools/microbench/lone_wave.hip).  The five kernel families around it:
//
//   blocks   mt_ streams with independent fixed-size blocks (hsrans_encode_device).  The reference's encoders are scalar CPU loops
//            (src/mt_rANS32x64_16w_encode.cpp:140-356); their only serial dependency between blocks is the coder state carried across
//            block boundaries.  With HSRANS_ENC_INDEPENDENT_BLOCKS every block starts from fresh states, so a block is one
//            self-contained job:
//              K_hist   k_block_histograms: byte counts of every block, a workgroup per block (32 LDS copies laid out [symbol][copy]: no
//                       bank conflicts)
//              K_enc    k_encode_blocks<S, CHUNK>: one wavefront per block, header [size][skip][states][counts]
//              K_gather k_gather_images adds up the image sizes in front of its block (K_scan, k_scan_images, does beyond 4,096 blocks),
//                       copies the image to its place; the last workgroup writes the file header [n][total] and the result words
//                       (page-locked host memory)
//              K_plan   k_plan_blocks: the sidecar plan, when asked for
//   raw      a whole raw stream is ONE dependent chain per coder state (hsrans_encode_device_raw): k_raw_histogram (wide) ->
//            k_encode_raw<S> (one wavefront; the image is the finished stream) -> k_copy_image (wide)
//   chain    block_ / mt_ streams whose states run through every block (hsrans_encode_device_ex): k_unit_summaries / k_unit_costs for
//            the host's block walk, then k_encode_chain<S> — one wavefront codes the blocks back to front and places the images — and
//            k_gather_chain
//   carried  the blocks are one slice of a longer stream (hsrans_encode_host_pipelined): K_hist and K_enc of `blocks`, then
//            k_scan_images_carried / k_gather_images_carried with the stream position carried from slice to slice, and
//            k_plan_blocks_carried after the last one
//   batch    many independent raw and mt_ streams, one launch per kernel kind (hsrans_encode_device_batch): the k_*_batch kernels, which
//            read their member's parameters from a device table and run the single calls' bodies; many chain streams likewise
//            (hsrans_encode_device_ex_batch): k_unit_summaries_batch / k_unit_costs_batch, k_encode_chain_batch<S>, k_gather_chain_batch
//
// Every result is byte-identical to the host encoder's (hsrans_host.cpp encode()).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "hsrans_encode.h"
#include "hsrans_kernels.h"

#include "enc_common.h"
#include "enc_normalise.h"
#include "enc_pass.h"
#include "enc_place.h"
#include "enc_batch.h"

namespace hsrans
{

uint32_t encode_block_count(uint64_t n, uint64_t block, uint32_t S)
{
  // hsrans_host.cpp split_blocks: the last block absorbs a remainder shorter than one group
  uint64_t count = (n + block - 1) / block;
  if (count > 1 && n - (count - 1) * block < S)
    count--;
  return count > 0xFFFFFFFFull ? 0 : (uint32_t)count;
}

uint64_t encode_slot_bytes(uint64_t block, uint32_t S)
{
  // every symbol emits at most one 16-bit word; the last block can be up to S-1 symbols longer
  const uint64_t need = 2 * (block + S) + 16 + 4 * (uint64_t)S + 512;
  return (need + 511) / 512 * 512; // (a multiple of the encoder's flush segment)
}

hipError_t prepare_encode_kernels()
{
  const size_t lds_few = sizeof(WaveLdsT<kChunkFew>), lds_many = sizeof(WaveLdsT<kChunkMany>);
  const std::pair<const void *, size_t> kernels[] = {{(const void *)k_encode_blocks<64, kChunkFew>, lds_few},
                                                     {(const void *)k_encode_blocks<32, kChunkFew>, lds_few},
                                                     {(const void *)k_encode_blocks<64, kChunkMany>, lds_many},
                                                     {(const void *)k_encode_blocks<32, kChunkMany>, lds_many},
                                                     {(const void *)k_encode_raw<64>, lds_few},
                                                     {(const void *)k_encode_raw<32>, lds_few},
                                                     {(const void *)k_encode_chain<64>, lds_few},
                                                     {(const void *)k_encode_chain<32>, lds_few},
                                                     {(const void *)k_encode_raw_batch<64>, lds_few},
                                                     {(const void *)k_encode_raw_batch<32>, lds_few},
                                                     {(const void *)k_encode_blocks_batch<64, kChunkFew>, lds_few},
                                                     {(const void *)k_encode_blocks_batch<32, kChunkFew>, lds_few},
                                                     {(const void *)k_encode_blocks_batch<64, kChunkMany>, lds_many},
                                                     {(const void *)k_encode_blocks_batch<32, kChunkMany>, lds_many},
                                                     {(const void *)k_encode_chain_batch<64>, lds_few},
                                                     {(const void *)k_encode_chain_batch<32>, lds_few}};
  for (const auto &k : kernels)
  {
    const hipError_t e = hipFuncSetAttribute(k.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.second);
    if (e != hipSuccess)
      return e;
  }
  return hipSuccess;
}

namespace
{
// One of the two chunk instantiations of a block kernel, and its LDS bytes, for a launch of `blocks` mt_ blocks in all.  Few blocks:
// all resident at once with the large chunks too (11 workgroups of 13.25 KiB per CU: the LDS is handed out in pieces); beyond, the
// small chunks (enc_common.h: kChunkFew, kChunkMany)
template <class Kernel>
struct ChunkVariant
{
  Kernel kernel;
  size_t lds;
};
template <class Kernel>
ChunkVariant<Kernel> chunk_variant(uint32_t blocks, uint32_t cus, Kernel with_few, Kernel with_many)
{
  if (blocks <= 11u * cus)
    return {with_few, sizeof(WaveLdsT<kChunkFew>)};
  return {with_many, sizeof(WaveLdsT<kChunkMany>)};
}

// K_hist -> K_enc of launch_encode and launch_encode_slice (the launches queued; errors are read by the caller)
void launch_encode_blocks(const EncParams &ep, uint32_t cus, hipStream_t stream)
{
  const auto enc = ep.S == 64 ? chunk_variant(ep.n_blocks, cus, k_encode_blocks<64, kChunkFew>, k_encode_blocks<64, kChunkMany>)
                              : chunk_variant(ep.n_blocks, cus, k_encode_blocks<32, kChunkFew>, k_encode_blocks<32, kChunkMany>);
  (void)hipGetLastError(); // (sticky per thread)
  if (ep.raw_counts != nullptr)
    hipLaunchKernelGGL(k_block_histograms, dim3(ep.n_blocks), dim3(256), 0, stream, ep, const_cast<uint32_t *>(ep.raw_counts));
  hipLaunchKernelGGL(enc.kernel, dim3(ep.n_blocks), dim3(64), enc.lds, stream, ep);
}
} // namespace

hipError_t launch_encode(const EncParams &ep, uint32_t cus, hipStream_t stream)
{
  launch_encode_blocks(ep, cus, stream);
  if (ep.n_blocks > kSelfScanBlocks)
    hipLaunchKernelGGL(k_scan_images, dim3(1), dim3(1024), 0, stream, ep);
  hipLaunchKernelGGL(k_gather_images, dim3(ep.n_blocks), dim3(256), 0, stream, ep);
  return hipGetLastError();
}

hipError_t launch_encode_slice(const EncParams &ep, EncCarry *carry, bool last_slice, uint8_t *heads, uint32_t cus, hipStream_t stream)
{
  launch_encode_blocks(ep, cus, stream);
  hipLaunchKernelGGL(k_scan_images_carried, dim3(1), dim3(1024), 0, stream, ep, carry, last_slice ? 1u : 0u);
  hipLaunchKernelGGL(k_gather_images_carried, dim3(ep.n_blocks), dim3(256), 0, stream, ep, heads);
  return hipGetLastError();
}

hipError_t launch_encode_raw(const EncParams &ep, uint32_t *d_counts, hipStream_t stream)
{
  const size_t lds = sizeof(WaveLdsT<kChunkFew>);
  (void)hipGetLastError();
  {
    // (also with the caller's histogram: the coding wavefront checks that every symbol that occurs has a slot in it)
    hipError_t e = hipMemsetAsync(d_counts, 0, 256 * 4, stream);
    if (e != hipSuccess)
      return e;
    const uint64_t per_wg = 1 << 16; // 16 passes of a workgroup's 4 KiB
    const uint32_t grid = (uint32_t)std::min<uint64_t>((ep.n + per_wg - 1) / per_wg, 4096);
    hipLaunchKernelGGL(k_raw_histogram, dim3(grid ? grid : 1), dim3(256), 0, stream, ep.in, ep.n, d_counts);
  }
  if (ep.S == 64)
    hipLaunchKernelGGL(k_encode_raw<64>, dim3(1), dim3(64), lds, stream, ep);
  else
    hipLaunchKernelGGL(k_encode_raw<32>, dim3(1), dim3(64), lds, stream, ep);
  hipLaunchKernelGGL(k_copy_image, dim3(1024), dim3(256), 0, stream, ep);
  return hipGetLastError();
}

hipError_t launch_unit_summaries(const EncParams &ep, void *summaries, const float *log_table, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_unit_summaries, dim3(ep.n_blocks), dim3(256), 0, stream, ep, (uint8_t *)summaries);
  if (log_table != nullptr)
    hipLaunchKernelGGL(k_unit_costs, dim3(ep.n_blocks), dim3(64), 0, stream, ep, (uint8_t *)summaries, log_table);
  return hipGetLastError();
}

hipError_t launch_encode_chain(const EncParams &ep, hipStream_t stream)
{
  const size_t lds = sizeof(WaveLdsT<kChunkFew>);
  (void)hipGetLastError();
  if (ep.S == 64)
    hipLaunchKernelGGL(k_encode_chain<64>, dim3(1), dim3(64), lds, stream, ep);
  else
    hipLaunchKernelGGL(k_encode_chain<32>, dim3(1), dim3(64), lds, stream, ep);
  // parts per image: from the largest slot (ep.slot_bytes here)
  const uint32_t parts = chain_gather_parts(ep.slot_bytes);
  hipLaunchKernelGGL(k_gather_chain, dim3(ep.n_blocks, parts), dim3(256), 0, stream, ep);
  return hipGetLastError();
}

hipError_t launch_unit_summaries_batch(const EncParams *params, const EncTask *unit_tasks, uint32_t n_unit_tasks, const EncTask *cost_tasks, uint32_t n_cost_tasks,
                                       uint8_t *const *summaries, const float *const *log_tables, hipStream_t stream, uint32_t *launches)
{
  (void)hipGetLastError();
  uint32_t n = 0;
  if (n_unit_tasks != 0)
  {
    hipLaunchKernelGGL(k_unit_summaries_batch, dim3(n_unit_tasks), dim3(256), 0, stream, params, unit_tasks, summaries);
    n++;
  }
  if (n_cost_tasks != 0)
  {
    hipLaunchKernelGGL(k_unit_costs_batch, dim3(n_cost_tasks), dim3(64), 0, stream, params, cost_tasks, summaries, log_tables);
    n++;
  }
  if (launches)
    *launches += n;
  return hipGetLastError();
}

hipError_t launch_encode_chain_batch(const EncParams *params, const uint32_t *members, uint32_t n64, uint32_t n32, const EncGatherTask *gather, uint32_t n_gather,
                                     hipStream_t stream, uint32_t *launches)
{
  const size_t lds = sizeof(WaveLdsT<kChunkFew>);
  (void)hipGetLastError();
  uint32_t n = 0;
  if (n64 != 0)
  {
    hipLaunchKernelGGL(k_encode_chain_batch<64>, dim3(n64), dim3(64), lds, stream, params, members);
    n++;
  }
  if (n32 != 0)
  {
    hipLaunchKernelGGL(k_encode_chain_batch<32>, dim3(n32), dim3(64), lds, stream, params, members + n64);
    n++;
  }
  if (n_gather != 0)
  {
    hipLaunchKernelGGL(k_gather_chain_batch, dim3(n_gather), dim3(256), 0, stream, params, gather);
    n++;
  }
  if (launches)
    *launches += n;
  return hipGetLastError();
}

hipError_t launch_encode_plan(const EncParams &ep, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_plan_blocks, dim3(ep.n_blocks), dim3(64), 0, stream, ep);
  return hipGetLastError();
}

hipError_t launch_encode_plan_carried(const EncParams &ep, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_plan_blocks_carried, dim3(ep.n_blocks), dim3(64), 0, stream, ep);
  return hipGetLastError();
}

hipError_t launch_encode_batch(const EncBatch &bt, uint32_t cus, hipStream_t stream, uint32_t *launches)
{
  const size_t lds_few = sizeof(WaveLdsT<kChunkFew>);
  const uint32_t n_mt = bt.n_mt64_blocks + bt.n_mt32_blocks;
  // the chunk variant from all mt_ blocks of the batch, as launch_encode picks it from one stream's
  const auto enc64 = chunk_variant(n_mt, cus, k_encode_blocks_batch<64, kChunkFew>, k_encode_blocks_batch<64, kChunkMany>);
  const auto enc32 = chunk_variant(n_mt, cus, k_encode_blocks_batch<32, kChunkFew>, k_encode_blocks_batch<32, kChunkMany>);
  uint32_t n = 0;
  (void)hipGetLastError(); // (sticky per thread)
  if (bt.zero_bytes != 0)
  {
    const hipError_t e = hipMemsetAsync(bt.zero, 0, bt.zero_bytes, stream);
    if (e != hipSuccess)
      return e;
  }
  // one launch of `kernel` over `grid` workgroups when that is not 0
  auto launch = [&](auto kernel, uint32_t grid, uint32_t threads, size_t lds, auto... args) {
    if (grid == 0)
      return;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, stream, args...);
    n++;
  };
  const EncTask *mt32 = bt.mt_blocks + bt.n_mt64_blocks;
  launch(k_raw_histogram_batch, bt.n_raw_parts, 256, 0, bt.params, bt.raw_parts);
  launch(k_block_histograms_batch, n_mt, 256, 0, bt.params, bt.mt_blocks);
  launch(k_encode_raw_batch<64>, bt.n_raw64, 64, lds_few, bt.params, bt.raw_members);
  launch(k_encode_raw_batch<32>, bt.n_raw32, 64, lds_few, bt.params, bt.raw_members + bt.n_raw64);
  launch(enc64.kernel, bt.n_mt64_blocks, 64, enc64.lds, bt.params, bt.mt_blocks);
  launch(enc32.kernel, bt.n_mt32_blocks, 64, enc32.lds, bt.params, mt32);
  launch(k_scan_images_batch, bt.n_scan, 1024, 0, bt.params, bt.scan_members);
  launch(k_gather_images_batch, n_mt, 256, 0, bt.params, bt.mt_blocks);
  launch(k_copy_images_batch, bt.n_raw_parts, 256, 0, bt.params, bt.raw_parts, bt.raw_headers);
  if (launches)
    *launches += n;
  return hipGetLastError();
}

hipError_t launch_encode_plan_batch(const EncParams *params, const EncTask *tasks, uint32_t n_tasks, hipStream_t stream, uint32_t *launches)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_plan_blocks_batch, dim3(n_tasks), dim3(64), 0, stream, params, tasks);
  if (launches)
    *launches += 1;
  return hipGetLastError();
}

} // namespace hsrans
