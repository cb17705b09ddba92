// enc_batch.h — hsrans_encode_device_batch and hsrans_encode_device_ex_batch: the _batch kernels, one launch per kernel kind over many streams.
// Part of the one encoder translation unit hsrans_encode.hip (which includes the parts in dependency order and holds the launchers).
#ifndef HSRANS_ENC_BATCH_H
#define HSRANS_ENC_BATCH_H

namespace hsrans
{
namespace
{

// ---- batches (hsrans_encode_device_batch): many independent streams, one launch per kernel kind ---------------------------
// Every member has an EncParams of its own in device memory (its slots, result words and checkpoints carved out of the context's
// buffers by the host); a workgroup finds its member — and the block or part of it — in a task list.  The members' parameters are
// read before anything is stored, so the compiler takes them with scalar loads (what a kernel argument costs) and the per-wave work
// is the single calls' own code: encode_body and the bodies above.
template <uint32_t S>
__global__ void __launch_bounds__(64) k_encode_raw_batch(const EncParams *__restrict__ params, const uint32_t *__restrict__ members)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const EncParams ep = params[members[blockIdx.x]];
  encode_body<S, true, kChunkFew>(ep, 0, *(WaveLdsT<kChunkFew> *)lds_raw, lane_id());
}

template <uint32_t S, uint32_t CHUNK>
__global__ void __launch_bounds__(64) k_encode_blocks_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  encode_body<S, false, CHUNK>(ep, t.index, *(WaveLdsT<CHUNK> *)lds_raw, lane_id());
}

// raw members: part t.index of t.count workgroups counts the member's bytes into its raw_counts (zeroed by the launcher)
__global__ void __launch_bounds__(256) k_raw_histogram_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ parts)
{
  const EncTask t = parts[blockIdx.x];
  const EncParams ep = params[t.member];
  raw_histogram_body(ep.in, ep.n, const_cast<uint32_t *>(ep.raw_counts), t.index, t.count);
}

// mt_ members: block t.index of member t.member
__global__ void __launch_bounds__(256) k_block_histograms_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks)
{
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  block_histograms_body(ep, t.index, const_cast<uint32_t *>(ep.raw_counts));
}

// mt_ members of more than kSelfScanBlocks blocks, one workgroup each
__global__ void __launch_bounds__(1024) k_scan_images_batch(const EncParams *__restrict__ params, const uint32_t *__restrict__ members)
{
  const EncParams ep = params[members[blockIdx.x]];
  scan_images_body(ep);
}

__global__ void __launch_bounds__(256) k_gather_images_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks)
{
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  gather_images_body(ep, t.index);
}

// raw members: part t.index of t.count workgroups copies the member's image; part 0 also puts the stream header (counts, final states)
// at headers[member] when that is not null, where the host fetches every member's header and checkpoints with one copy
__global__ void __launch_bounds__(256) k_copy_images_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ parts, uint8_t *const *__restrict__ headers)
{
  const EncTask t = parts[blockIdx.x];
  const EncParams ep = params[t.member];
  uint8_t *header = headers[t.member];
  copy_image_body(ep, t.index, t.count);
  if (t.index != 0 || header == nullptr || ep.result[1] == 0)
    return;
  const uint8_t *src = ep.scratch + ep.slot_bytes - ep.image_bytes[0]; // (2-byte aligned)
  for (uint32_t i = threadIdx.x * 2; i < 16 + 512 + 4 * ep.S; i += 512)
    *(uint16_t *)(header + i) = *(const uint16_t *)(src + i);
}

// mt_ members that asked for a plan (ep.plan set by the host once the chain counts are known); the others' blocks return at once
__global__ void __launch_bounds__(64) k_plan_blocks_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks)
{
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  if (ep.plan == nullptr)
    return;
  plan_blocks_body(ep, t.index);
}

// ---- batches of chain encodes (hsrans_encode_device_ex_batch): block_ / mt_ streams whose states run through every block -----------
// What differs between members and a kernel argument cannot carry: where a member's summaries go and which logarithm table its bit
// width reads — pointer arrays by member, as k_copy_images_batch takes `headers` — and its unit size, ep.block of its own record.

// unit t.index of member t.member into summaries[t.member]
__global__ void __launch_bounds__(256) k_unit_summaries_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks, uint8_t *const *__restrict__ summaries)
{
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  uint8_t *mine = summaries[t.member];
  unit_summaries_body(ep, t.index, mine);
}

// the adaptive members' whole units: unit t.index of member t.member, with the table of the member's bit width
__global__ void __launch_bounds__(64) k_unit_costs_batch(const EncParams *__restrict__ params, const EncTask *__restrict__ tasks, uint8_t *const *__restrict__ summaries,
                                                         const float *const *__restrict__ log_tables)
{
  const EncTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  uint8_t *mine = summaries[t.member];
  const float *table = log_tables[t.member];
  unit_costs_body(ep, lane_id(), t.index, mine, table);
}

// A pointer read from a member's record is a generic one, and what is loaded through a generic pointer counts as different from lane
// to lane: the chain loop reads its block records that way and steers its scalar word cursor by them.  A pointer that is a kernel
// argument is known to point to device memory; this says the same of the record's.
template <class T>
__device__ __forceinline__ T *device_memory(T *p)
{
  __attribute__((address_space(1))) T *g = (__attribute__((address_space(1))) T *)p;
  asm volatile("" : "+s"(g)); // (no instruction: keeps the two casts from being folded into none)
  return (T *)g;
}
__device__ __forceinline__ EncParams chain_params_in_device_memory(EncParams ep)
{
  ep.in = device_memory(ep.in);
  ep.out = device_memory(ep.out);
  ep.scratch = device_memory(ep.scratch);
  ep.image_bytes = device_memory(ep.image_bytes);
  ep.image_off = device_memory(ep.image_off);
  ep.result = device_memory(ep.result);
  ep.ck_states = device_memory(ep.ck_states);
  ep.ck_pos = device_memory(ep.ck_pos);
  ep.given_counts = device_memory(ep.given_counts);
  ep.ck_groups = device_memory(ep.ck_groups);
  ep.chain_blocks = device_memory(ep.chain_blocks);
  ep.block_states = device_memory(ep.block_states);
  ep.stamps = device_memory(ep.stamps);
  return ep;
}

// one workgroup of one wavefront per member: its whole chain
template <uint32_t S>
__global__ void __launch_bounds__(64) k_encode_chain_batch(const EncParams *__restrict__ params, const uint32_t *__restrict__ members)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const EncParams ep = chain_params_in_device_memory(params[members[blockIdx.x]]);
  encode_chain_body<S>(ep, *(WaveLdsT<kChunkFew> *)lds_raw, lane_id());
}

// part t.part of t.parts of image t.block of member t.member
__global__ void __launch_bounds__(256) k_gather_chain_batch(const EncParams *__restrict__ params, const EncGatherTask *__restrict__ tasks)
{
  const EncGatherTask t = tasks[blockIdx.x];
  const EncParams ep = params[t.member];
  gather_chain_body(ep, t.block, t.part, t.parts);
}

} // namespace
} // namespace hsrans

#endif
