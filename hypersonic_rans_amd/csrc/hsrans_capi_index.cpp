// hsrans_capi_index.cpp — sidecar indexes of existing streams: hsrans_index_build[_at], hsrans_decode_device_indexing (first decode that leaves its index behind).
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h); split out of hsrans_capi.cpp in round 5 by concern.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <memory>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_index_groups.h"
#include "hsrans_cpu.h"
#include "hsrans_encode.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"
#include "hsrans_batch.h"


extern "C"
{

// Where the blocks of an index come from: a base plan's single-piece chains (raw, mt_), or the records of the walk over a block_ stream —
// block b's {header position, output offset, header word} in blocks[3b .. 3b+2] and the states it was entered with in bstates[b * S ..]
struct IndexSource
{
  uint32_t n_blocks;
  const uint32_t *cf0, *st0; // base plan
  const Piece *pc0;
  const uint64_t *blocks; // walk records (null: a base plan)
  const uint32_t *bstates;
  uint64_t decoded_len;
};
static IndexSource source_of_plan(const uint8_t *base, const PlanHeader &h)
{
  return {h.n_chains, (const uint32_t *)(base + plan_chain_first_off()), (const uint32_t *)(base + plan_states_off(h.n_chains, h.n_pieces)),
          (const Piece *)(base + plan_pieces_off(h.n_chains)), nullptr, nullptr, h.decoded_len};
}

// The chains of a plan with a checkpoint every `interval` groups, given what a recording pass left at the checkpoints (slot = absolute
// group / interval): one fill chain per single-symbol block, one chain per block start and per checkpoint inside a coded block (IndexBlock,
// hsrans_kernels.h: the fill kernels write the same on the device).  false: no plan (a tail behind a trailing single-symbol block).
static bool add_interval_chains(PlanBuilder &pb, const IndexSource &src, uint32_t interval, const uint32_t *ck_states, const uint64_t *ck_words)
{
  const uint32_t S = pb.hdr.states;
  for (uint32_t b = 0; b < src.n_blocks; b++)
  {
    const bool last = b + 1 == src.n_blocks;
    const uint64_t *rec = src.blocks ? src.blocks + 3 * (size_t)b : nullptr;
    const Piece *bp = rec ? nullptr : &src.pc0[src.cf0[b]];
    const IndexBlock blk = rec ? index_block_of_walk(rec[0], rec[1], rec[2], src.decoded_len, S, last) : index_block_of_piece(*bp, S, last);
    const uint32_t *entry = rec ? src.bstates + (size_t)b * S : src.st0 + (size_t)bp->state_idx * S;
    if (rec && index_block_ends_short(blk, src.decoded_len))
      return false;
    for (uint32_t k = 0, n = index_block_chains(blk, interval); k < n; k++)
      pb.add_chain(index_chain_piece(blk, S, interval, k, ck_words, 0), index_chain_states(blk, S, interval, k, entry, ck_states));
  }
  return true;
}

// ---- what every recording pass shares ------------------------------------------------------------------------------------------------
// (PassBytes, PassBuffers, pass_bytes and walk_max_blocks — what a recording pass writes besides the output — are in hsrans_internal.h: the batch's too)

// The pass: the base plan (blob and status word on the device, header h) decodes d_stream into d_out and records {states, read cursor} every
// `interval` groups, or (interval 0) at the n_groups ascending groups of d_groups; a walk plan also records its blocks.
static hipError_t launch_recording_pass(hsrans_ctx *ctx, const uint8_t *d_plan, uint32_t *d_status, const PlanHeader &h, const void *d_stream, size_t stream_length,
                                        void *d_out, size_t out_capacity, uint32_t interval, const uint64_t *d_groups, uint32_t n_groups, const PassBuffers &b, hipStream_t s)
{
  KParams kp{};
  kp.stream = (const uint8_t *)d_stream;
  kp.stream_len = stream_length;
  kp.out = (uint8_t *)d_out;
  kp.out_cap = out_capacity;
  kp.plan = d_plan;
  kp.status = d_status;
  kp.ckpt_states = b.ck_states;
  kp.ckpt_words = b.ck_words;
  kp.ckpt_interval = interval;
  kp.ckpt_groups = d_groups;
  kp.n_ckpt_groups = n_groups;
  kp.walk_blocks = b.walk_blocks;
  kp.walk_states = b.walk_states;
  kp.walk_count = b.walk_count;
  kp.walk_max_blocks = b.max_blocks;
  PlanHeader hl = h;
  if (!(h.flags & kPlanWalk))
    hl.shared_hist = 0; // private tables: every chain of the pass builds its own (raw has one chain, mt_ one per block)
  return launch_decode(ctx->tuning, kp, hl, ctx->geom, s, nullptr);
}

// The status word a pass left, once it is on the host: non-zero (a bad histogram / header) is reported and cleared like hsrans_dplan_status does
static int pass_status_rc(uint32_t status, uint32_t *d_status, hipStream_t s)
{
  if (status == 0)
    return HSRANS_OK;
  return hipMemsetAsync(d_status, 0, 4, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess ? HSRANS_E_DEVICE : HSRANS_E_HIP;
}

// What a recording walk left, brought down to host_ck [checkpoint states | cursors] and host_walk [blocks | entry states] (sized by pbytes):
// the count and the status word first, then as many blocks and entry states as there are and the checkpoints, with one more synchronisation
static int download_walk_records(const PassBuffers &b, const PassBytes &pbytes, uint32_t S, uint32_t *d_status, uint8_t *host_ck, uint8_t *host_walk, uint32_t *n_blocks,
                                 hipStream_t s)
{
  uint32_t status = 0xFFFFFFFF;
  *n_blocks = 0;
  if (hipMemcpyAsync(n_blocks, b.walk_count, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  if (status != 0)
    return pass_status_rc(status, d_status, s);
  if (*n_blocks == 0 || *n_blocks > b.max_blocks)
    return HSRANS_E_FORMAT;
  if (hipMemcpyAsync(host_ck, b.ck_states, pbytes.st, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(host_ck + pbytes.st, b.ck_words, pbytes.wd, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(host_walk, b.walk_blocks, (size_t)*n_blocks * 24, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(host_walk + pbytes.blk, b.walk_states, (size_t)*n_blocks * S * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}
// ... and the plan's chains from that copy
static bool add_walk_chains(PlanBuilder &pb, const PassBytes &pbytes, const uint8_t *host_ck, const uint8_t *host_walk, uint32_t n_blocks, uint32_t interval)
{
  const IndexSource src{n_blocks, nullptr, nullptr, nullptr, (const uint64_t *)host_walk, (const uint32_t *)(host_walk + pbytes.blk), pb.hdr.decoded_len};
  return add_interval_chains(pb, src, interval, (const uint32_t *)host_ck, (const uint64_t *)(host_ck + pbytes.st));
}

static size_t index_build_impl(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint32_t index_interval,
                               const uint64_t *groups, size_t n_groups, uint8_t *plan_out, size_t plan_capacity)
{
  // One pass over an existing stream that records {states, read cursor} every `index_interval` groups inside every rANS piece of the
  // stream's own plan; the checkpoints then become additional chains.  raw: one dependent chain, indexed on the host (below).  mt_: one
  // wavefront per block, in parallel.  A block_ stream is one chain with inline headers (the position of a block's header is only known
  // once the block before it is decoded): the single wavefront that walks it also reports every block header it meets and the states it
  // enters the block with, and the plan gets one chain per block plus the checkpoints.
  if (ctx == nullptr || in == nullptr || plan_out == nullptr || !valid_codec(container, states, bits))
    return 0;
  // checkpoints every index_interval groups, or (groups != nullptr) at explicit ascending group indices
  if (groups == nullptr && (index_interval == 0 || index_interval % 4 != 0))
    return 0;
  if (in_length < 16)
    return 0;
  if (groups != nullptr)
  {
    index_interval = 0;
    if (n_groups == 0 || n_groups > 0xFFFFFFFFull || container == HSRANS_BLOCK || !index_groups_valid(groups, n_groups))
      return 0;
  }
  uint64_t out_len;
  memcpy(&out_len, in, 8);
  // (the header's decoded length is untrusted: the base plan is sized by the chains the stream really holds, at most ~40x the stream)
  std::vector<uint8_t> base;
  if (!plan_build_vec(container, states, bits, in, in_length, (size_t)out_len, &base))
    return 0;
  const size_t base_size = base.size();
  PlanHeader h;
  memcpy(&h, base.data(), sizeof(h));
  const IndexSource src = source_of_plan(base.data(), h);
  const uint32_t S = (uint32_t)states;
  const bool walk = (h.flags & kPlanWalk) != 0;
  if (!walk && h.n_pieces != h.n_chains) // the planner only produces single-piece chains for raw and mt_
    return 0;
  // A raw stream is one dependent chain: one wavefront records its checkpoints at ~0.65 GB/s, one host core with this
  // library's SIMD decoder at 2-3 GB/s and without the upload — so raw streams are indexed on the host (same plan, byte for
  // byte).  mt_ blocks (one wavefront each, in parallel) and block_ streams
  // (the walk that also reports the inline headers) stay on the GPU.
  if (container == HSRANS_RAW)
  {
    std::vector<uint64_t> own;
    if (groups == nullptr)
    {
      const uint64_t T = h.n_pieces == 1 ? src.pc0[0].steps : 0;
      for (uint64_t g = index_interval; g < T; g += index_interval)
        own.push_back(g);
      if (own.empty())
        return plan_capacity >= base_size ? (memcpy(plan_out, base.data(), base_size), base_size) : 0;
    }
    return cpu::index_build(cpu::best_level(), 1, container, states, bits, in, in_length, groups ? groups : own.data(), groups ? n_groups : own.size(), plan_out,
                            plan_capacity, groups ? 0 : index_interval);
  }
  const uint64_t n_ck = groups ? n_groups : out_len / S / index_interval + 2;
  const uint64_t max_blocks = walk ? std::min<uint64_t>(walk_max_blocks(out_len), 0xFFFFFFFFull) : 0;
  const PassBytes pbytes = pass_bytes(n_ck, S, max_blocks);

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return 0;
  const size_t in_pad = up16(in_length);
  if (!grow(&ctx->d_in, &ctx->d_in_cap, in_pad) || !grow(&ctx->d_out, &ctx->d_out_cap, (size_t)out_len + 16) || !grow(&ctx->d_plan, &ctx->d_plan_cap, base_size))
    return 0;
  // one region for what the pass records, for this call only: [checkpoint states | cursors | the caller's groups | blocks | entry states | block count]
  const size_t off_wd = up16(pbytes.st), off_groups = off_wd + up16(pbytes.wd), off_blk = off_groups + up16(groups ? n_groups * 8 : 0), off_bst = off_blk + up16(pbytes.blk);
  const size_t off_count = off_bst + up16(pbytes.bst);
  uint8_t *d_rec = nullptr;
  if (hipMalloc((void **)&d_rec, off_count + 16) != hipSuccess)
  {
    (void)hipGetLastError();
    return 0;
  }
  const PassBuffers pass{(uint32_t *)d_rec, (uint64_t *)(d_rec + off_wd), walk ? (uint64_t *)(d_rec + off_blk) : nullptr, walk ? (uint32_t *)(d_rec + off_bst) : nullptr,
                         walk ? (uint32_t *)(d_rec + off_count) : nullptr, (uint32_t)max_blocks};
  uint64_t *d_groups = groups ? (uint64_t *)(d_rec + off_groups) : nullptr;
  size_t result = 0;
  hipStream_t s = ctx->stream;
  std::vector<uint8_t> host_ck(pbytes.st + pbytes.wd);                        // the records on the host: [checkpoint states | cursors]
  std::unique_ptr<uint8_t[]> host_walk(new uint8_t[pbytes.blk + pbytes.bst]); // ... and the walk's [blocks | entry states]
  const uint32_t *ck_states = (const uint32_t *)host_ck.data();
  const uint64_t *ck_words = (const uint64_t *)(host_ck.data() + pbytes.st);
  do
  {
    if (groups && hipMemcpyAsync(d_groups, groups, n_groups * 8, hipMemcpyHostToDevice, s) != hipSuccess)
      break;
    if (hipMemsetAsync(d_rec + off_count, 0, 16, s) != hipSuccess || hipMemcpyAsync(ctx->d_in, in, in_length, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(ctx->d_plan, base.data(), base_size, hipMemcpyHostToDevice, s) != hipSuccess || hipMemsetAsync(ctx->d_status, 0, 4, s) != hipSuccess)
      break;
    if (launch_recording_pass(ctx, ctx->d_plan, ctx->d_status, h, ctx->d_in, in_length, ctx->d_out, out_len, index_interval, d_groups, (uint32_t)(groups ? n_groups : 0), pass,
                              s) != hipSuccess)
      break;
    PlanBuilder pb;
    pb.begin(container, states, bits, out_len, in_length);
    pb.hdr.interval = index_interval;
    if (walk)
    {
      uint32_t n_blocks = 0;
      if (download_walk_records(pass, pbytes, S, ctx->d_status, host_ck.data(), host_walk.get(), &n_blocks, s) != HSRANS_OK ||
          !add_walk_chains(pb, pbytes, host_ck.data(), host_walk.get(), n_blocks, index_interval))
        break;
    }
    else
    {
      uint32_t status = 0xFFFFFFFF;
      if (hipMemcpyAsync(host_ck.data(), pass.ck_states, pbytes.st, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(host_ck.data() + pbytes.st, pass.ck_words, pbytes.wd, hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(&status, ctx->d_status, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
          pass_status_rc(status, ctx->d_status, s) != HSRANS_OK)
        break;
      if (groups != nullptr)
        add_group_chains(pb, h, src.cf0, src.pc0, src.st0, groups, n_groups, ck_states, ck_words);
      else
        add_interval_chains(pb, src, index_interval, ck_states, ck_words);
    }
    result = pb.serialize(plan_out, plan_capacity);
  } while (false);
  if (result == 0)
  {
    (void)hipStreamSynchronize(s); // nothing queued above may still be using the region when it is freed
    (void)hipGetLastError();
  }
  (void)hipFree(d_rec);
  return result;
}

size_t hsrans_index_build(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint32_t index_interval,
                          uint8_t *plan_out, size_t plan_capacity)
try
{
  return index_build_impl(ctx, container, states, bits, in, in_length, index_interval, nullptr, 0, plan_out, plan_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_index_build_at(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, const uint64_t *groups,
                             size_t n_groups, uint8_t *plan_out, size_t plan_capacity)
try
{
  if (groups == nullptr)
    return 0;
  return index_build_impl(ctx, container, states, bits, in, in_length, 0, groups, n_groups, plan_out, plan_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

// ---- what both device assemblies share ----------------------------------------------------------------------------------------------
// The checkpoint buffers of a first decode: the context's (the GPU encoder's, kept and grown; under ctx->lock), not fresh allocations
static bool context_checkpoints(hsrans_ctx *ctx, const PassBytes &pbytes, PassBuffers *b)
{
  if (!grow(&ctx->d_enc_ck, &ctx->d_enc_ck_cap, pbytes.st + pbytes.wd))
    return false;
  b->ck_states = (uint32_t *)ctx->d_enc_ck;
  b->ck_words = (uint64_t *)(ctx->d_enc_ck + pbytes.st);
  return true;
}

// (hsrans_internal.h: the plan a device assembly writes, and its arena's scratch)
extern "C++" hsrans_dplan *assembly_plan(hsrans_ctx *ctx, uint32_t S, uint32_t max_chains, size_t max_groups, size_t off_words, size_t extra, hipStream_t s, uint8_t **scratch)
{
  hsrans_dplan *nd = dplan_new(ctx);
  if (nd == nullptr)
    return nullptr;
  DplanRegions r;
  r.counters = true;
  r.plan = (size_t)plan_size(max_chains, max_chains, S, 0);
  r.groups = max_groups * sizeof(Group);
  r.scratch = kAssemblyOffsets + up16(off_words * 4) + extra;
  r.zero = kZeroAll;
  if (dplan_arena(nd, r, s, scratch) != HSRANS_OK)
  {
    hsrans_dplan_destroy(nd);
    return nullptr;
  }
  return nd;
}

// finish_assembly's halves (hsrans_internal.h), to run around one synchronisation
extern "C++" bool assembly_copy_down(const hsrans_dplan *d, const IndexResult *d_result, hipStream_t s, IndexResult *r, uint32_t *status)
{
  return hipMemcpyAsync(r, d_result, sizeof(*r), hipMemcpyDeviceToHost, s) == hipSuccess && hipMemcpyAsync(status, d->d_status, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
}
extern "C++" int assembly_adopt(const hsrans_dplan *d, hsrans_dplan *nd, int rc, const IndexResult &r, uint32_t interval, uint32_t min_chains, uint32_t max_chains,
                                uint32_t max_groups, hipStream_t s, const Group *host_groups)
{
  // no plan: IndexResult::error, no chains, or more chains / groups than the arena has room for
  if (rc == HSRANS_OK && (r.error != 0 || r.chains < min_chains || r.chains > max_chains || r.groups > max_groups))
    rc = HSRANS_E_FORMAT;
  if (rc != HSRANS_OK)
  {
    (void)hipGetLastError();
    hsrans_dplan_destroy(nd);
    return rc;
  }
  PlanHeader hn = d->hdr;
  hn.flags = 0;
  hn.n_chains = hn.n_pieces = r.chains;
  hn.interval = interval;
  hn.shared_hist = r.coded == 1 ? 1 : 0;
  hn.aux_off = hn.shared_hist ? r.hist_off : 0;
  dplan_adopt(nd, hn, r.groups, r.fewest, s, host_groups); // (kIndexNoFewest is the largest spread_min_block a plan keeps)
  return HSRANS_OK;
}

// Behind the pass and the assembly kernels (`queued`: all of them were): what the count kernel left comes back with the base plan d's status
// word, is checked against the bounds, and nd takes over the plan the device wrote.  One synchronisation — nothing queued may still be running
// when this returns, whatever failed; on failure nd is destroyed.
static int finish_assembly(hsrans_dplan *d, hsrans_dplan *nd, bool queued, const IndexResult *d_result, uint32_t interval, uint32_t min_chains, uint32_t max_chains,
                           uint32_t max_groups, hipStream_t s, IndexResult *r)
{
  uint32_t status = 0xFFFFFFFF;
  const bool ok = queued && assembly_copy_down(d, d_result, s, r, &status);
  const bool synced = hipStreamSynchronize(s) == hipSuccess;
  return assembly_adopt(d, nd, ok && synced ? pass_status_rc(status, d->d_status, s) : HSRANS_E_HIP, *r, interval, min_chains, max_chains, max_groups, s);
}

// The sizes of a block_ member's first decode, its pass buffers and the arguments of its assembly kernels (hsrans_internal.h)
extern "C++" bool walk_assembly_sizes(const PlanHeader &h, uint32_t interval, WalkAssemblySizes *z)
{
  z->n_ck = pass_checkpoints(h.decoded_len, h.states, interval);
  z->max_blocks = walk_max_blocks(h.decoded_len);
  z->max_chains = z->max_blocks + z->n_ck;
  z->max_groups = z->max_blocks + z->max_chains / kGroupPartChains + 16;
  z->pbytes = pass_bytes(z->n_ck, h.states, z->max_blocks);
  return z->max_chains <= 0xFFFFFFF0u;
}
extern "C++" void walk_assembly_args(const hsrans_ctx *ctx, const hsrans_dplan *d, const hsrans_dplan *nd, uint8_t *scratch, uint32_t interval, const WalkAssemblySizes &z,
                                     PassBuffers *pass, WalkIndexArgs *wa)
{
  const PlanHeader &h = d->hdr;
  uint32_t *d_offsets = (uint32_t *)(scratch + kAssemblyOffsets);
  pass->walk_count = (uint32_t *)(scratch + kAssemblyCount);
  pass->walk_blocks = (uint64_t *)(scratch + kAssemblyOffsets + up16(2 * (size_t)z.max_blocks * 4));
  pass->walk_states = (uint32_t *)((uint8_t *)pass->walk_blocks + z.pbytes.blk);
  pass->max_blocks = (uint32_t)z.max_blocks;
  *wa = WalkIndexArgs{};
  wa->base = d->d_plan;
  wa->walk_count = pass->walk_count;
  wa->walk_blocks = pass->walk_blocks;
  wa->walk_states = pass->walk_states;
  wa->ck_states = pass->ck_states;
  wa->ck_words = pass->ck_words;
  wa->S = h.states;
  wa->interval = interval;
  wa->max_blocks = (uint32_t)z.max_blocks;
  wa->max_chains = (uint32_t)z.max_chains;
  wa->max_groups = (uint32_t)z.max_groups;
  wa->parts_want = kGroupPartsPerCU * ctx->geom.num_cus;
  wa->decoded_len = h.decoded_len;
  wa->stream_len = h.stream_len;
  wa->chain_off = d_offsets;
  wa->group_off = d_offsets + z.max_blocks;
  wa->result = (IndexResult *)scratch;
  wa->plan = nd->d_plan;
  wa->groups = (Group *)nd->d_groups;
}
// ... and an mt_ member's
extern "C++" MtAssemblySizes mt_assembly_sizes(const hsrans_ctx *ctx, const PlanHeader &h, uint32_t interval)
{
  MtAssemblySizes z{};
  z.n_ck = pass_checkpoints(h.decoded_len, h.states, interval);
  z.pbytes = pass_bytes(z.n_ck, h.states, 0);
  z.max_chains = (uint32_t)std::min<uint64_t>((uint64_t)h.n_chains + z.n_ck, 0xFFFFFFF0u);
  // at most one group per block, and where there are few every block's chains in parts of >= kGroupPartChains chains (as dplan_fill)
  z.max_groups = (uint32_t)std::min<uint64_t>((uint64_t)h.n_chains + z.max_chains / kGroupPartChains + 16, 0xFFFFFFF0u);
  return z;
}
extern "C++" void mt_assembly_args(const hsrans_ctx *ctx, const hsrans_dplan *d, const hsrans_dplan *nd, uint8_t *scratch, uint32_t interval, const MtAssemblySizes &z, const PassBuffers &pass,
                                   IndexArgs *ia)
{
  *ia = IndexArgs{};
  ia->base = d->d_plan;
  ia->n_base = d->hdr.n_chains;
  ia->S = d->hdr.states;
  ia->interval = interval;
  ia->ck_states = pass.ck_states;
  ia->ck_words = pass.ck_words;
  ia->chain_off = (uint32_t *)(scratch + kAssemblyOffsets);
  ia->group_off = ia->chain_off + d->hdr.n_chains;
  ia->result = (IndexResult *)scratch;
  ia->plan = nd->d_plan;
  ia->max_chains = z.max_chains;
  ia->max_groups = z.max_groups;
  ia->groups = (Group *)nd->d_groups;
  ia->parts_want = kGroupPartsPerCU * ctx->geom.num_cus;
  ia->stream_len = d->hdr.stream_len;
}

// hsrans_decode_device_indexing for a block_ stream's walk plan (d: kPlanWalk, one chain, no checkpoints; the arguments are checked).  The one
// wavefront that walks the inline headers decodes into the caller's d_out and records block headers, entry states and checkpoints; behind it,
// on the same stream, k_walk_index_count / k_walk_index_fill write the indexed plan and its group list into the new plan's arena, which also
// holds the walk's records.  HSRANS_INDEX_ASSEMBLE_ON_HOST=1: the records come down and add_interval_chains + hsrans_dplan_create make the same plan.
static int decode_walk_indexing(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                                uint32_t index_interval, hipStream_t s, hsrans_dplan **indexed, bool have_lock)
{
  const PlanHeader &h = d->hdr;
  const uint32_t S = h.states;
  WalkAssemblySizes z;
  if (!walk_assembly_sizes(h, index_interval, &z))
    return HSRANS_E_FORMAT;
  const uint64_t n_ck = z.n_ck, max_chains = z.max_chains, max_groups = z.max_groups;
  std::unique_lock<std::mutex> guard(ctx->lock, std::defer_lock); // (the checkpoint buffer belongs to the context)
  if (!have_lock)
    guard.lock();
  const PassBytes &pbytes = z.pbytes;
  PassBuffers pass{};
  if (!context_checkpoints(ctx, pbytes, &pass))
    return HSRANS_E_HIP;
  uint8_t *scratch = nullptr;
  hsrans_dplan *nd = assembly_plan(ctx, S, (uint32_t)max_chains, (size_t)max_groups, 2 * (size_t)z.max_blocks, pbytes.blk + pbytes.bst, s, &scratch);
  if (nd == nullptr)
    return HSRANS_E_HIP;
  WalkIndexArgs wa;
  walk_assembly_args(ctx, d, nd, scratch, index_interval, z, &pass, &wa);
  const bool passed = launch_recording_pass(ctx, d->d_plan, d->d_status, h, d_stream, stream_length, d_out, out_capacity, index_interval, nullptr, 0, pass, s) == hipSuccess;

  if (passed && ctx->tuning.index_assemble_on_host)
  {
    uint32_t n_blocks = 0;
    const int rc = grow_pinned(&ctx->h_pin, &ctx->h_pin_cap, pbytes.all()) ? download_walk_records(pass, pbytes, S, d->d_status, ctx->h_pin, ctx->h_pin + pbytes.st + pbytes.wd, &n_blocks, s) : HSRANS_E_HIP;
    if (rc != HSRANS_OK)
      (void)hipStreamSynchronize(s), (void)hipGetLastError(); // (nothing queued here may still be running when the call returns, whatever failed)
    hsrans_dplan_destroy(nd); // (it only lent its arena to the walk's records)
    if (rc != HSRANS_OK)
      return rc;
    PlanBuilder pb;
    pb.begin((int)h.container, (int)S, h.bits, h.decoded_len, h.stream_len);
    pb.reserve((size_t)n_blocks + n_ck);
    pb.hdr.interval = index_interval;
    if (!add_walk_chains(pb, pbytes, ctx->h_pin, ctx->h_pin + pbytes.st + pbytes.wd, n_blocks, index_interval))
      return HSRANS_E_FORMAT;
    std::vector<uint8_t> plan(pb.serialized_size());
    const size_t plan_bytes = pb.serialize(plan.data(), plan.size());
    return plan_bytes == 0 ? HSRANS_E_FORMAT : hsrans_dplan_create(ctx, plan.data(), plan_bytes, indexed);
  }

  IndexResult res{};
  const int rc = finish_assembly(d, nd, passed && launch_index_assemble_walk(wa, s) == hipSuccess, wa.result, index_interval, 1, (uint32_t)max_chains, (uint32_t)max_groups, s, &res);
  if (rc != HSRANS_OK)
    return rc;
  if (ctx->tuning.indexing_trace)
    fprintf(stderr, "hsrans_decode_device_indexing: block_ on the device: %u blocks, %u chains, %u groups, %zu plan bytes\n", res.blocks, res.chains, res.groups, nd->plan_bytes);
  *indexed = nd;
  return HSRANS_OK;
}

// The first decode of a stream that came without an index (a reference-emitted mt_ stream planned by hsrans_plan_build or on the
// device by hsrans_dplan_create_from_device_stream: one chain per block, most wave slots empty) also RECORDS the coder states and
// the read cursor every `index_interval` groups — two stores per checkpoint on a pass that is latency-bound anyway — and returns
// the plan with those checkpoints for every later decode of the same stream.  The stream never leaves device memory; the plan
// blob (chain table, a few MB) equals hsrans_index_build's byte for byte: mt_ and block_ plans are assembled on the device behind the pass,
// raw plans on the host.  A block_ stream comes with its walk plan (hsrans_plan_build, or hsrans_dplan_create_from_device_stream from the
// stream's head): decode_walk_indexing.
int hsrans_decode_device_indexing(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                                  uint32_t index_interval, void *hip_stream, hsrans_dplan **indexed)
{
  return decode_device_indexing_impl(ctx, d, d_stream, stream_length, d_out, out_capacity, index_interval, hip_stream, indexed, false);
}

// have_lock: the caller (hsrans_decode_host) already holds ctx->lock
extern "C++" int decode_device_indexing_impl(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                                       uint32_t index_interval, void *hip_stream, hsrans_dplan **indexed, bool have_lock)
try
{
  if (indexed == nullptr)
    return HSRANS_E_ARG;
  *indexed = nullptr;
  const int checked = indexing_args_check(ctx, d, d_stream, stream_length, d_out, out_capacity, index_interval);
  if (checked != HSRANS_OK)
    return checked;
  const PlanHeader &h = d->hdr;
  const bool walk = (h.flags & kPlanWalk) != 0;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  if (walk)
    return decode_walk_indexing(ctx, d, d_stream, stream_length, d_out, out_capacity, index_interval, s, indexed, have_lock);
  const bool trace = ctx->tuning.indexing_trace;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  const uint32_t S = h.states;
  const MtAssemblySizes z = mt_assembly_sizes(ctx, h, index_interval);
  const uint64_t n_ck = z.n_ck;
  std::unique_lock<std::mutex> guard(ctx->lock, std::defer_lock); // (the checkpoint buffer and the staging belong to the context)
  if (!have_lock)
    guard.lock();
  const PassBytes &pbytes = z.pbytes;
  PassBuffers pass{};
  if (!context_checkpoints(ctx, pbytes, &pass))
    return HSRANS_E_HIP;
  const uint32_t max_chains = z.max_chains;
  // mt_ streams (one single-piece chain per block, histograms in the stream): the indexed plan is assembled ON THE DEVICE behind the
  // recording pass — one allocation, three launches, one synchronisation; nothing but an IndexResult comes back to the host
  // (HSRANS_INDEX_ASSEMBLE_ON_HOST=1: checkpoints down, blob built by one core, blob up — still what raw plans take)
  if (indexing_mt_on_device(h) && !ctx->tuning.index_assemble_on_host)
  {
    const uint32_t nb = h.n_chains;
    uint8_t *scratch = nullptr;
    hsrans_dplan *nd = assembly_plan(ctx, S, max_chains, z.max_groups, 2 * (size_t)nb, 0, s, &scratch);
    if (nd == nullptr)
      return HSRANS_E_HIP;
    IndexArgs ia;
    mt_assembly_args(ctx, d, nd, scratch, index_interval, z, pass, &ia);
    const bool queued = launch_recording_pass(ctx, d->d_plan, d->d_status, h, d_stream, stream_length, d_out, out_capacity, index_interval, nullptr, 0, pass, s) == hipSuccess &&
                        launch_index_assemble(ia, s) == hipSuccess;
    IndexResult res{};
    const int rc = finish_assembly(d, nd, queued, ia.result, index_interval, nb, max_chains, z.max_groups, s, &res);
    if (rc != HSRANS_OK)
      return rc;
    if (trace)
      fprintf(stderr, "hsrans_decode_device_indexing: on the device: %.3f ms in all (%u chains, %zu plan bytes)\n", ms(t0, now()), res.chains, nd->plan_bytes);
    *indexed = nd;
    return HSRANS_OK;
  }
  // page-locked staging (kept by the context): [checkpoint states | cursors | base plan] down, then the new plan blob up —
  // from pageable memory these copies (12.5 MB of states each way for 100 MB at 32 groups) took 15 ms, the decode 0.25
  const size_t base_bytes = up16(d->plan_bytes);
  const size_t new_cap = (size_t)plan_size(max_chains, max_chains, S, kPlanHasHist);
  if (!grow_pinned(&ctx->h_pin, &ctx->h_pin_cap, pbytes.all() + base_bytes + new_cap))
    return HSRANS_E_HIP;
  uint32_t *ck_states = (uint32_t *)ctx->h_pin;
  uint64_t *ck_words = (uint64_t *)(ctx->h_pin + pbytes.st);
  uint8_t *base = ctx->h_pin + pbytes.all();
  uint8_t *plan = base + base_bytes;
  size_t plan_bytes = 0;
  int rc = HSRANS_E_HIP;
  do
  {
    uint32_t status = 0xFFFFFFFF;
    if (launch_recording_pass(ctx, d->d_plan, d->d_status, h, d_stream, stream_length, d_out, out_capacity, index_interval, nullptr, 0, pass, s) != hipSuccess ||
        hipMemcpyAsync(base, d->d_plan, d->plan_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(ck_states, pass.ck_states, pbytes.st, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(ck_words, pass.ck_words, pbytes.wd, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&status, d->d_status, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      break;
    const auto t1 = now();
    if ((rc = pass_status_rc(status, d->d_status, s)) != HSRANS_OK)
      break;
    PlanHeader hb;
    if (!read_header(base, d->plan_bytes, &hb) || hb.n_chains != h.n_chains || hb.n_pieces != h.n_pieces || hb.states != h.states ||
        !plan_validate(base, d->plan_bytes, h.stream_len, h.decoded_len))
    {
      rc = HSRANS_E_FORMAT;
      break;
    }
    PlanBuilder pb;
    pb.begin((int)h.container, (int)S, h.bits, h.decoded_len, h.stream_len);
    pb.reserve((size_t)h.n_chains + n_ck);
    pb.hdr.interval = index_interval;
    if (hb.flags & kPlanHasHist)
    {
      uint16_t counts[256];
      memcpy(counts, base + plan_hist_off(hb.n_chains, hb.n_pieces, hb.states), 512);
      pb.set_hist(counts);
    }
    add_interval_chains(pb, source_of_plan(base, hb), index_interval, ck_states, ck_words);
    const auto t2 = now();
    plan_bytes = pb.serialize(plan, new_cap);
    rc = plan_bytes == 0 ? HSRANS_E_FORMAT : HSRANS_OK;
    if (trace)
      fprintf(stderr, "hsrans_decode_device_indexing: pass + copies %.3f ms, validate + chains %.3f ms, serialize %.3f ms (%zu bytes)\n", ms(t0, t1), ms(t1, t2), ms(t2, now()), plan_bytes);
  } while (false);
  if (rc != HSRANS_OK)
  {
    (void)hipStreamSynchronize(s); // nothing queued above may still be writing the staging buffers (or the caller's d_out) after the return
    (void)hipGetLastError();
    return rc;
  }
  const auto t3 = now();
  const int rc2 = hsrans_dplan_create(ctx, plan, plan_bytes, indexed);
  if (trace)
    fprintf(stderr, "hsrans_decode_device_indexing: hsrans_dplan_create %.3f ms\n", ms(t3, now()));
  return rc2;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}


} // extern "C"
