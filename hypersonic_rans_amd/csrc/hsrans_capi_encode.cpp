// hsrans_capi_encode.cpp — GPU encoder entries: hsrans_encode_device (mt_, one wavefront per block), hsrans_encode_device_raw,
// hsrans_encode_device_ex (every format hsrans_encode_ex writes); and the host side the batch and the host pipeline share with the
// single calls (declared in hsrans_internal.h): argument rules and shapes, per-block arrays, plan assembly, kernel setup, and the steps
// of the chain path (ex_route ... chain_plan_finish) that hsrans_encode_device_ex and hsrans_encode_device_ex_batch both run.
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
#include <new>
#include <utility>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_cpu.h"
#include "hsrans_encode.h"
#include "hsrans_index_groups.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"
#include "hsrans_batch.h"


namespace
{
// the block choice of a chain encode: unit summaries on the device (counts, the run that ends each unit, and for the adaptive policy
// every unit's own code length), the walk on the host (the host encoder's code).  Caller holds ctx->lock, device set.
bool device_block_walk(hsrans_ctx *ctx, ChainJob *job, hipStream_t s, double *summaries_us, double *walk_us)
{
  const auto t0 = std::chrono::steady_clock::now();
  if (!chain_units(job))
    return false;
  const bool fixed = job->fixed;
  const size_t n_units = job->n_units;
  std::vector<UnitSummary> units(n_units);
  std::vector<float> table(fixed ? 0 : (1u << job->bits) + 1);
  if (!fixed)
    walk_log_table(job->bits, table.data());
  const EncParams ep = chain_units_params(*job);
  Carve meta; // [summaries | logarithm table]
  meta.take(n_units * sizeof(UnitSummary));
  const size_t table_at = meta.take(table.size() * 4);
  if (!grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, meta.at))
    return false;
  const float *d_table = fixed ? nullptr : (const float *)(ctx->d_enc_meta + table_at);
  if ((!fixed && hipMemcpyAsync((void *)d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
      launch_unit_summaries(ep, ctx->d_enc_meta, d_table, s) != hipSuccess ||
      hipMemcpyAsync(units.data(), ctx->d_enc_meta, n_units * sizeof(UnitSummary), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  const auto t1 = std::chrono::steady_clock::now();
  if (!chain_walk(job, units.data()))
    return false;
  const auto t2 = std::chrono::steady_clock::now();
  *summaries_us = std::chrono::duration<double, std::micro>(t1 - t0).count();
  *walk_us = std::chrono::duration<double, std::micro>(t2 - t1).count();
  return true;
}

size_t copy_choices(const std::vector<BlockSpan> &spans, hsrans_block_choice *out, size_t capacity)
{
  for (size_t b = 0; b < spans.size() && b < capacity && out != nullptr; b++)
  {
    out[b].begin = spans[b].begin;
    out[b].end = spans[b].end;
    out[b].single = spans[b].single ? 1 : 0;
    out[b].symbol = spans[b].single ? spans[b].symbol : 0;
    if (spans[b].single)
      memset(out[b].counts, 0, 512);
    else
      memcpy(out[b].counts, spans[b].hist.symbolCount, 512);
  }
  return spans.size();
}
} // namespace

ExRoute ex_route(int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity, const hsrans_encode_opts *opts, ChainJob *job)
{
  if (!valid_codec(container, states, bits) || d_in == nullptr || d_out == nullptr || length == 0)
    return kExRefused;
  if (out_capacity < capacity(container, states, length) || ((uintptr_t)d_in & 15) != 0 || ((uintptr_t)d_out & 15) != 0)
    return kExRefused;
  ChainJob j;
  j.container = container;
  j.S = (uint32_t)states;
  j.bits = bits;
  j.d_in = d_in;
  j.length = length;
  j.d_out = d_out;
  j.out_capacity = out_capacity;
  j.ig = opts && opts->n_index_groups ? opts->index_groups : nullptr;
  j.n_ig = j.ig ? opts->n_index_groups : 0;
  j.interval = j.ig ? 0 : (opts ? opts->index_interval : 0);
  j.want_plan = j.interval != 0 || j.ig != nullptr;
  if ((j.want_plan && ((j.interval % 4) != 0 || opts->plan_out == nullptr)) || !index_groups_valid(j.ig, j.n_ig))
    return kExRefused;
  j.fixed = opts && opts->block_size != 0;
  j.independent = opts && (opts->flags & HSRANS_ENC_INDEPENDENT_BLOCKS) != 0;
  if (j.independent && (container != HSRANS_MT || !j.fixed))
    return kExRefused;
  j.block = j.fixed ? opts->block_size : 0;
  if (j.block % 64 != 0)
    return kExRefused;
  *job = std::move(j);
  if (container == HSRANS_RAW)
    return kExRaw;
  if (job->independent && !job->want_plan)
    return kExBlocks;
  if (job->independent && job->interval != 0)
    return kExBlocksPlan;
  // limits of the one-wavefront pass: byte offsets inside a block's slot are 32-bit (as the raw encoder's; a fixed block longer than the
  // input is the input: one block); listed checkpoints sit on set boundaries (4 groups) of a block, which fixed blocks of a group count
  // that is not a multiple of 4 do not keep
  if (length > 0x7FFF0000ull || (job->ig && job->fixed && (job->block / job->S) % 4 != 0))
    return kExRefused;
  return kExChain;
}

bool chain_units(ChainJob *job)
{
  job->unit = job->fixed ? job->block : walk_unit(job->container, job->S, job->bits);
  job->n_units = (job->length + job->unit - 1) / job->unit;
  return job->n_units <= 0xFFFFFFFFull;
}

EncParams chain_units_params(const ChainJob &job)
{
  EncParams ep{};
  ep.S = job.S;
  ep.bits = job.bits;
  ep.in = (const uint8_t *)job.d_in;
  ep.n = job.length;
  ep.block = job.unit;
  ep.n_blocks = (uint32_t)job.n_units;
  return ep;
}

bool chain_walk(ChainJob *job, const UnitSummary *units)
{
  return job->fixed ? fixed_blocks(job->length, job->block, job->S, job->bits, units, &job->spans)
                    : reference_blocks(job->container, job->length, job->S, job->bits, units, &job->spans);
}

void chain_prepare(ChainJob *job)
{
  const std::vector<BlockSpan> &spans = job->spans;
  const uint32_t S = job->S, interval = job->interval;
  const size_t nb = spans.size(), length = job->length;
  const uint64_t T = length + 1 >= S ? (length - S + 1 + S - 1) / S : 0; // whole groups of the file
  std::vector<ChainBlock> &cb = job->cb;
  cb.assign(nb, ChainBlock{});
  job->counts.assign(nb * 256, 0);
  uint64_t slot_at = 0, slot_max = 0;
  uint32_t n_ck = 0;
  for (size_t b = 0; b < nb; b++)
  {
    const BlockSpan &sp = spans[b];
    ChainBlock &c = cb[b];
    c.begin = sp.begin;
    c.end = sp.end;
    c.slot_bytes = sp.single ? 512 : encode_slot_bytes(sp.end - sp.begin, S);
    slot_at += c.slot_bytes;
    slot_max = std::max<uint64_t>(slot_max, c.slot_bytes);
    c.slot_end = slot_at;
    c.single = sp.single ? 0x100u | sp.symbol : 0;
    c.ck_base = n_ck;
    if (!sp.single)
    {
      memcpy(&job->counts[b * 256], sp.hist.symbolCount, 512);
      const uint64_t whole = (sp.end - sp.begin) / S;
      if (interval != 0 && whole >= 1)
        n_ck += (uint32_t)((whole - 1) / interval);
    }
  }
  // listed checkpoints: the entries the host encoder meets (inside a coded block, not its first group, below T), and their blocks
  std::vector<uint32_t> &ck_list = job->ck_list;
  std::vector<uint32_t> &ck_block = job->ck_block; // (interval checkpoints too: the block of every checkpoint slot)
  ck_list.clear();
  ck_block.clear();
  if (job->ig)
  {
    const uint64_t *ig = job->ig;
    size_t b = 0;
    for (size_t k = 0; k < job->n_ig && ig[k] < T; k++)
    {
      while (b < nb && (spans[b].end - 1) / S < ig[k])
        b++;
      if (b == nb)
        break;
      if (!spans[b].single && ig[k] > spans[b].begin / S)
      {
        ck_list.push_back((uint32_t)ig[k]);
        ck_block.push_back((uint32_t)b);
      }
    }
    n_ck = (uint32_t)ck_list.size();
  }
  else if (job->want_plan)
  {
    ck_block.reserve(n_ck);
    for (size_t b = 0; b < nb; b++)
    {
      const uint32_t next = b + 1 < nb ? cb[b + 1].ck_base : n_ck;
      for (uint32_t k = cb[b].ck_base; k < next; k++)
        ck_block.push_back((uint32_t)b);
    }
  }
  job->n_ck = n_ck;
  job->slot_total = slot_at;
  job->slot_max = slot_max;
}

ChainDown chain_down_layout(const ChainJob &job)
{
  const size_t nb = job.spans.size();
  Carve at;
  ChainDown d;
  d.image_bytes = at.take(nb * 8);
  d.image_off = at.take(nb * 8);
  d.result = at.take(256);
  d.bytes = at.at;
  return d;
}

ChainUp chain_up_layout(const ChainJob &job)
{
  const size_t nb = job.spans.size();
  Carve at;
  ChainUp u;
  u.blocks = at.take(nb * sizeof(ChainBlock));
  u.counts = at.take(nb * 512);
  u.list = at.take(job.ck_list.size() * 4 + 4);
  u.bytes = at.close();
  return u;
}

ChainCk chain_ck_layout(const ChainJob &job)
{
  const size_t ck_slots = job.n_ck ? job.n_ck : 1;
  Carve words; // (32-bit words, packed: the states and positions as ck_region lays them, then the block states)
  ChainCk c;
  words.take(ck_slots * job.S, 1);
  c.ck_pos = words.take(ck_slots, 1);
  c.block_states = words.take(job.want_plan ? job.spans.size() * (size_t)job.S : 0, 1);
  c.bytes = words.at * 4;
  return c;
}

void chain_up_fill(const ChainJob &job, uint8_t *host_up)
{
  const ChainUp u = chain_up_layout(job);
  memcpy(host_up + u.blocks, job.cb.data(), job.cb.size() * sizeof(ChainBlock));
  memcpy(host_up + u.counts, job.counts.data(), job.counts.size() * 2);
  if (!job.ck_list.empty())
    memcpy(host_up + u.list, job.ck_list.data(), job.ck_list.size() * 4);
}

EncParams chain_params(const ChainJob &job, uint8_t *d_scratch, uint8_t *d_down, uint8_t *d_up, uint8_t *d_ck)
{
  const ChainDown down = chain_down_layout(job);
  const ChainUp up = chain_up_layout(job);
  const ChainCk ck = chain_ck_layout(job);
  EncParams ep{};
  ep.S = job.S;
  ep.bits = job.bits;
  ep.in = (const uint8_t *)job.d_in;
  ep.n = job.length;
  ep.out = (uint8_t *)job.d_out;
  ep.out_cap = job.out_capacity;
  ep.scratch = d_scratch;
  ep.slot_bytes = job.slot_max;
  ep.n_blocks = (uint32_t)job.spans.size();
  ep.image_bytes = (uint64_t *)(d_down + down.image_bytes);
  ep.image_off = (uint64_t *)(d_down + down.image_off);
  ep.result = (uint64_t *)(d_down + down.result);
  ep.chain_blocks = (const ChainBlock *)(d_up + up.blocks);
  ep.given_counts = (const uint16_t *)(d_up + up.counts);
  ep.ck_groups = job.ck_list.empty() ? nullptr : (const uint32_t *)(d_up + up.list);
  ep.n_ck_groups = (uint32_t)job.ck_list.size();
  ep.interval = job.want_plan ? job.interval : 0;
  ep.ck_states = (uint32_t *)d_ck;
  ep.ck_pos = ep.ck_states + ck.ck_pos;
  ep.block_states = job.want_plan ? ep.ck_states + ck.block_states : nullptr;
  ep.chain_mt = job.container == HSRANS_MT ? 1 : 0;
  ep.chain_independent = job.independent ? 1 : 0;
  return ep;
}

size_t chain_plan_bytes(const ChainJob &job)
{
  // blocks_plan_from_checkpoints: one chain per block and one per checkpoint, every chain a single piece, no histogram copy
  const uint64_t chains = (uint64_t)job.spans.size() + job.n_ck;
  return chains > 0xFFFFFFFFull ? ~(size_t)0 : (size_t)plan_size((uint32_t)chains, (uint32_t)chains, job.S, 0);
}

size_t chain_plan_finish(const ChainJob &job, uint64_t total, const uint64_t *img_bytes, const uint64_t *img_off, const uint32_t *blk_states, const uint32_t *ck_states,
                         const uint32_t *ck_pos, uint8_t *plan_out, size_t plan_capacity)
{
  const std::vector<BlockSpan> &spans = job.spans;
  const uint32_t S = job.S, n_ck = job.n_ck;
  const size_t nb = spans.size();
  const uint64_t counts_at = job.container == HSRANS_MT ? 16 + 4 * (uint64_t)S : 8; // the counts inside a coded block's image
  std::vector<EncodedBlock> blocks(nb);
  for (size_t b = 0; b < nb; b++)
    blocks[b] = EncodedBlock{spans[b].begin, spans[b].end, spans[b].single, spans[b].symbol, total - (img_off[b] + counts_at + 512),
                             total - (img_off[b] + counts_at), &blk_states[b * S]};
  std::vector<uint64_t> ck_group(n_ck), ck_wfe(n_ck);
  for (uint32_t k = 0; k < n_ck; k++)
  {
    const uint32_t b = job.ck_block[k];
    ck_group[k] = job.ig ? job.ck_list[k] : spans[b].begin / S + (uint64_t)(k - job.cb[b].ck_base + 1) * job.interval;
    ck_wfe[k] = total - (img_off[b] + img_bytes[b]) + ck_pos[k]; // (ck_pos: bytes from the cursor to the end of the block's words)
  }
  return blocks_plan_from_checkpoints(job.container, (int)S, job.bits, job.length, total, job.interval, blocks.data(), nb, n_ck, ck_group.data(), ck_wfe.data(), ck_states,
                                      plan_out, plan_capacity);
}

bool encoder_ready(hsrans_ctx *ctx)
{
  if (hipSetDevice(ctx->device) != hipSuccess)
    return false;
  if (!ctx->encoder_prepared && prepare_encode_kernels() == hipSuccess)
    ctx->encoder_prepared = true;
  return ctx->encoder_prepared;
}

bool encoder_buffers(hsrans_ctx *ctx, size_t scratch, size_t meta, size_t ck)
{
  return grow(&ctx->d_enc_scratch, &ctx->d_enc_scratch_cap, scratch) && grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, meta) &&
         grow(&ctx->d_enc_ck, &ctx->d_enc_ck_cap, ck);
}

void ck_region(EncParams *ep, uint8_t *at, size_t ck_slots, uint32_t S)
{
  ep->ck_states = (uint32_t *)at;
  ep->ck_pos = ep->ck_states + ck_slots * S;
}

bool stream_settle(hipStream_t s, bool queued)
{
  if (hipStreamSynchronize(s) == hipSuccess && queued)
    return true;
  (void)hipGetLastError();
  return false;
}

EncParams EncShape::params(const void *d_in, void *d_out, size_t out_capacity) const
{
  EncParams ep{};
  ep.S = S;
  ep.bits = bits;
  ep.in = (const uint8_t *)d_in;
  ep.n = n;
  ep.out = (uint8_t *)d_out;
  ep.out_cap = out_capacity;
  ep.block = block;
  ep.n_blocks = n_blocks;
  ep.slot_bytes = slot_bytes;
  ep.interval = interval;
  ep.max_ck = max_ck;
  return ep;
}

bool raw_shape(int states, uint32_t bits, size_t length, size_t out_capacity, const hsrans_hist *hist, uint32_t index_interval, const uint64_t *index_groups,
               size_t n_index_groups, bool plan, EncShape *sh)
{
  EncShape r;
  r.listed = index_groups != nullptr && n_index_groups != 0;
  if (!valid_codec(HSRANS_RAW, states, bits) || length == 0 || length > 0x7FFF0000ull || index_interval % 4 != 0 || // (byte offsets inside the slot are 32-bit)
      out_capacity < capacity(HSRANS_RAW, states, length) || (r.listed && (n_index_groups > 0x7FFFFFFFull || !index_groups_valid(index_groups, n_index_groups))))
    return false;
  if (hist != nullptr)
  {
    uint32_t sum = 0;
    for (int k = 0; k < 256; k++)
      sum += hist->symbolCount[k];
    if (sum != (1u << bits))
      return false;
  }
  r.S = (uint32_t)states;
  r.bits = bits;
  r.n = r.block = length;
  r.want_plan = plan && (r.listed || index_interval != 0);
  // checkpoints the pass will record: interval -> group (k + 1) * interval; list -> the entries below the last whole group
  const uint64_t whole_groups = length / r.S;
  if (r.want_plan && r.listed)
    while (r.n_ck < n_index_groups && index_groups[r.n_ck] < whole_groups)
      r.n_ck++;
  else if (r.want_plan)
    r.n_ck = whole_groups >= 1 ? (size_t)((whole_groups - 1) / index_interval) : 0;
  r.slot_bytes = encode_slot_bytes(length, r.S);
  r.interval = r.want_plan && !r.listed ? index_interval : 0;
  r.max_ck = (uint32_t)r.n_ck;
  r.ck_slots = r.n_ck ? r.n_ck : 1;
  *sh = r;
  return true;
}

bool mt_shape(int states, uint32_t bits, size_t length, size_t out_capacity, uint32_t block_size, uint32_t index_interval, bool plan, EncShape *sh)
{
  if (!valid_codec(HSRANS_MT, states, bits) || length == 0 || block_size == 0 || block_size % 64 != 0 || block_size > (1u << 30) || index_interval % 4 != 0 ||
      out_capacity < capacity(HSRANS_MT, states, length)) // (same contract as the host encoders)
    return false;
  EncShape r;
  r.S = (uint32_t)states;
  r.bits = bits;
  r.n = length;
  r.block = block_size;
  r.n_blocks = encode_block_count(length, block_size, r.S);
  if (r.n_blocks == 0)
    return false;
  r.slot_bytes = encode_slot_bytes(block_size, r.S);
  r.interval = plan ? index_interval : 0; // checkpoints only serve the plan
  r.max_ck = r.interval ? (block_size / r.S - 1) / r.interval : 0;
  r.ck_slots = (size_t)r.n_blocks * (r.max_ck ? r.max_ck : 1);
  *sh = r;
  return true;
}

size_t mt_block_arrays_bytes(uint32_t n_blocks) { return ((size_t)n_blocks * 24 + 15) / 16 * 16 + 16 + (size_t)n_blocks * 1024; }

void mt_block_arrays(EncParams *ep, uint8_t *at)
{
  const size_t nb = ep->n_blocks;
  ep->image_bytes = (uint64_t *)at;
  ep->image_off = ep->image_bytes + nb;
  ep->chain_count = (uint32_t *)(ep->image_off + nb);
  ep->chain_off = ep->chain_count + nb;
  ep->fits = (uint64_t *)(at + (nb * 24 + 15) / 16 * 16);
  ep->raw_counts = (const uint32_t *)(ep->fits + 2);
}

bool mt_result_header(const EncParams &ep, const uint64_t *result, PlanHeader *h)
{
  if (result[2] == 0 || result[2] > 0xFFFFFFFFull)
    return false;
  *h = mt_plan_header(ep.S, ep.bits, ep.n, result[0], (uint32_t)result[2]);
  h->shared_hist = result[3] == 1 ? 1 : 0; // exactly one block with a histogram (hsrans_host.cpp PlanBuilder::serialize)
  h->aux_off = h->shared_hist ? result[4] : 0;
  h->interval = ep.interval;
  return true;
}

namespace
{
// the plan is decoded by the grouped launch (blocks with checkpoints), for which K_plan writes the group list
bool mt_grouped(const EncParams &ep, const PlanHeader &h) { return ep.interval != 0 && ep.n_blocks < h.n_chains; }
} // namespace

hsrans_dplan *mt_plan_begin(hsrans_ctx *ctx, EncParams *ep, const uint64_t *result, PlanHeader *h, hipStream_t s)
{
  hsrans_dplan *d = mt_result_header(*ep, result, h) ? dplan_new(ctx) : nullptr;
  if (d == nullptr)
    return nullptr;
  const bool grouped = mt_grouped(*ep, *h);
  // few large blocks: every block's chains in parts (every coded block but the last has max_ck + 1 chains; at most 64 parts a block)
  ep->group_split = grouped ? group_parts_of(ep->max_ck + 1, std::min(group_parts_max(ctx->geom, ep->n_blocks), 64u)) : 1;
  // ONE device allocation for the status word, the ticket counters of the dynamic group order (as dplan_fill; without them the launch
  // falls back to the static order), the plan and the group list, one memset over the first three, one synchronisation (round 4:
  // up to four hipMalloc, three memsets, three synchronisations — 0.14 ms on top of a 0.2 ms encode)
  DplanRegions r;
  r.counters = grouped;
  r.plan = (size_t)plan_size(h->n_chains, h->n_pieces, h->states, 0);
  r.groups = grouped ? (size_t)ep->n_blocks * ep->group_split * sizeof(Group) : 0;
  r.zero = kZeroThroughPlan;
  if (dplan_arena(d, r, s) != HSRANS_OK || hipMemcpyAsync(d->d_plan, h, sizeof(*h), hipMemcpyHostToDevice, s) != hipSuccess)
  {
    hsrans_dplan_destroy(d);
    return nullptr;
  }
  ep->plan = d->d_plan;
  ep->groups = d->d_groups;
  ep->n_chains = h->n_chains;
  return d;
}

void mt_plan_adopt(hsrans_dplan *d, const EncParams &ep, const PlanHeader &h, hipStream_t s)
{
  dplan_adopt(d, h, mt_grouped(ep, h) ? ep.n_blocks * ep.group_split : 0, ep.max_ck + 1, s);
}

size_t raw_plan(hsrans_ctx *ctx, const EncShape &sh, uint64_t total, const uint64_t *index_groups, const uint8_t *header, const uint32_t *ck_states,
                const uint32_t *ck_pos, uint8_t *plan_out, size_t plan_capacity, size_t *plan_size, hsrans_dplan **out_dplan)
{
  std::vector<uint64_t> ck_group(sh.n_ck), ck_wfe(sh.n_ck);
  for (size_t k = 0; k < sh.n_ck; k++)
  {
    ck_group[k] = sh.listed ? index_groups[k] : (uint64_t)(k + 1) * sh.interval;
    ck_wfe[k] = ck_pos[k];
  }
  std::vector<uint8_t> own(plan_out ? 0 : plan_capacity_chains(HSRANS_RAW, (int)sh.S, sh.n, sh.n_ck, 0));
  uint8_t *blob = plan_out ? plan_out : own.data();
  const size_t psize = raw_plan_from_checkpoints((int)sh.S, sh.bits, sh.n, total, (const uint16_t *)(header + 16), (const uint32_t *)(header + 16 + 512), sh.n_ck,
                                                 ck_group.data(), ck_wfe.data(), ck_states, sh.interval, blob, plan_out ? plan_capacity : own.size());
  if (psize == 0)
    return 0;
  if (plan_size)
    *plan_size = psize;
  if (out_dplan != nullptr && hsrans_dplan_create(ctx, blob, psize, out_dplan) != HSRANS_OK)
    return 0;
  return psize;
}

extern "C"
{

size_t hsrans_block_choices(int container, int states, uint32_t bits, const void *in, size_t length, uint32_t block_size, hsrans_block_choice *out, size_t capacity)
try
{
  if ((container != HSRANS_BLOCK && container != HSRANS_MT) || !valid_codec(container, states, bits) || in == nullptr || length == 0 || block_size % 64 != 0)
    return 0;
  const size_t unit = block_size ? block_size : walk_unit(container, (uint32_t)states, bits);
  std::vector<UnitSummary> units((length + unit - 1) / unit);
  unit_summaries((const uint8_t *)in, length, unit, units.data());
  std::vector<BlockSpan> spans;
  if (block_size == 0)
    unit_fresh_costs(container, length, (uint32_t)states, bits, units.data());
  if (!(block_size ? fixed_blocks(length, block_size, (uint32_t)states, bits, units.data(), &spans)
                   : reference_blocks(container, length, (uint32_t)states, bits, units.data(), &spans)))
    return 0;
  return copy_choices(spans, out, capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_block_choices_device(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, uint32_t block_size,
                                   hsrans_block_choice *out, size_t capacity, void *hip_stream)
try
{
  if (ctx == nullptr || (container != HSRANS_BLOCK && container != HSRANS_MT) || !valid_codec(container, states, bits) || d_in == nullptr || length == 0 ||
      block_size % 64 != 0 || ((uintptr_t)d_in & 15) != 0 || length > 0x7FFF0000ull)
    return 0;
  std::lock_guard<std::mutex> guard(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return 0;
  ChainJob job;
  job.container = container;
  job.S = (uint32_t)states;
  job.bits = bits;
  job.d_in = d_in;
  job.length = length;
  job.block = block_size;
  job.fixed = block_size != 0;
  double a = 0, b = 0;
  if (!device_block_walk(ctx, &job, (hipStream_t)hip_stream, &a, &b))
    return 0;
  return copy_choices(job.spans, out, capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_encode_device_raw(hsrans_ctx *ctx, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity, const hsrans_hist *hist,
                                uint32_t index_interval, const uint64_t *index_groups, size_t n_index_groups, uint8_t *plan_out, size_t plan_capacity,
                                size_t *plan_size, void *hip_stream, hsrans_dplan **out_dplan)
try
{
  // SURVEY.md §8(f) row 2, the raw half: rANS32x64_16w.cpp:34-166 carries every coder state from the file's last symbol to its
  // first, so the format has work for exactly ONE wavefront (lane j = state j).  What the GPU adds is that input and stream never
  // leave HBM: a wide kernel counts the bytes, the coding wavefront normalises them exactly as hist.cpp:16-215 does, codes the file
  // back to front through an LDS ring with its table entries fetched two sets ahead, records the checkpoints of the sidecar index
  // on its way, and a wide copy puts the finished image at the front of d_out.  Byte-identical to hsrans_encode_ex (tests).
  if (out_dplan)
    *out_dplan = nullptr;
  if (plan_size)
    *plan_size = 0;
  EncShape sh;
  if (ctx == nullptr || !device_io_ok(d_in, d_out) || (plan_out != nullptr && plan_size == nullptr) ||
      !raw_shape(states, bits, length, out_capacity, hist, index_interval, index_groups, n_index_groups, plan_out != nullptr || out_dplan != nullptr, &sh))
    return 0;
  const size_t n_ck = sh.n_ck;
  std::vector<uint32_t> groups32(sh.want_plan && sh.listed ? n_ck : 0);
  for (size_t k = 0; k < groups32.size(); k++)
    groups32[k] = (uint32_t)index_groups[k];
  EncParams ep = sh.params(d_in, d_out, out_capacity);
  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return 0;
  const size_t meta_bytes = (2 + kEncResultWords + 4) * 8 + 256 * 4 + 256 * 2 + n_ck * 4 + 64;
  if (!encoder_buffers(ctx, ep.slot_bytes, meta_bytes, ck_region_bytes(sh.ck_slots, sh.S)))
    return 0;
  ep.scratch = ctx->d_enc_scratch;
  ep.image_bytes = (uint64_t *)ctx->d_enc_meta;
  ep.image_off = ep.image_bytes + 1;
  ep.result = ep.image_off + 1;
  ep.stamps = ep.result + kEncResultWords;
  uint32_t *d_counts = (uint32_t *)(ep.stamps + 4);
  uint16_t *d_given = (uint16_t *)(d_counts + 256);
  uint32_t *d_groups = (uint32_t *)(d_given + 256);
  ep.raw_counts = d_counts;
  ep.given_counts = hist ? d_given : nullptr;
  ep.ck_groups = groups32.empty() ? nullptr : d_groups;
  ep.n_ck_groups = (uint32_t)groups32.size();
  ck_region(&ep, ctx->d_enc_ck, sh.ck_slots, sh.S);
  hipStream_t s = (hipStream_t)hip_stream;
  uint64_t result[kEncResultWords] = {};
  bool ok = true;
  if (hist)
    ok = hipMemcpyAsync(d_given, hist->symbolCount, 512, hipMemcpyHostToDevice, s) == hipSuccess;
  if (ok && ep.ck_groups)
    ok = hipMemcpyAsync(d_groups, groups32.data(), n_ck * 4, hipMemcpyHostToDevice, s) == hipSuccess;
  ok = ok && launch_encode_raw(ep, d_counts, s) == hipSuccess && hipMemcpyAsync(result, ep.result, sizeof(result), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (!stream_settle(s, ok)) // (groups32 / *hist may be read until here)
    return 0;
  if (ctx->tuning.debug_stamps)
  {
    uint64_t st[4] = {};
    if (hipMemcpy(st, ep.stamps, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "[hsrans raw encode stamps] us: counts+normalise+table %.1f  rANS pass %.1f\n", (double)(st[2] - st[0]) / 100.0, (double)(st[3] - st[2]) / 100.0);
  }
  if (!enc_result_ok(result, true))
    return 0;
  const size_t total = (size_t)result[0];
  if (!sh.want_plan)
    return total;

  // ---- the sidecar plan: checkpoints and the stream's header come down (2.1 MB for the one-chain-per-wavefront index), the host
  // assembles exactly what hsrans_encode_ex emits ----
  std::vector<uint8_t> header(16 + 512 + 4 * (size_t)sh.S);
  std::vector<uint32_t> ck_states(n_ck * sh.S), ck_pos(n_ck);
  if (hipMemcpy(header.data(), d_out, header.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      (n_ck && (hipMemcpy(ck_states.data(), ep.ck_states, n_ck * sh.S * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(ck_pos.data(), ep.ck_pos, n_ck * 4, hipMemcpyDeviceToHost) != hipSuccess)))
    return 0;
  return raw_plan(ctx, sh, total, index_groups, header.data(), ck_states.data(), ck_pos.data(), plan_out, plan_capacity, plan_size, out_dplan) ? total : 0;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_encode_device(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity,
                            uint32_t block_size, uint32_t index_interval, void *hip_stream, hsrans_dplan **out_dplan)
try
{
  if (container == HSRANS_RAW) // one wavefront (the format's one dependent chain); block_size has no meaning
    return hsrans_encode_device_raw(ctx, states, bits, d_in, length, d_out, out_capacity, nullptr, index_interval, nullptr, 0, nullptr, 0, nullptr, hip_stream, out_dplan);
  if (out_dplan)
    *out_dplan = nullptr;
  EncShape sh;
  if (ctx == nullptr || container != HSRANS_MT || !device_io_ok(d_in, d_out) ||
      !mt_shape(states, bits, length, out_capacity, block_size, index_interval, out_dplan != nullptr, &sh))
    return 0;
  EncParams ep = sh.params(d_in, d_out, out_capacity);
  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return 0;
  const bool stamps = ctx->tuning.debug_stamps;
  const size_t nb = ep.n_blocks, arrays = mt_block_arrays_bytes(ep.n_blocks);
  if (!encoder_buffers(ctx, nb * ep.slot_bytes, arrays + (stamps ? nb * 4 * 8 : 0), ck_region_bytes(sh.ck_slots, sh.S)))
    return 0;
  ep.scratch = ctx->d_enc_scratch;
  mt_block_arrays(&ep, ctx->d_enc_meta);
  ep.stamps = stamps ? (uint64_t *)(ctx->d_enc_meta + arrays) : nullptr;
  // the result words land in page-locked host memory the kernels write directly (the stream is synchronised before they are read)
  if (ctx->h_enc_result == nullptr && hipHostMalloc((void **)&ctx->h_enc_result, kEncResultWords * 8, hipHostMallocMapped) != hipSuccess)
  {
    ctx->h_enc_result = nullptr;
    return 0;
  }
  void *d_result = nullptr;
  if (hipHostGetDevicePointer(&d_result, ctx->h_enc_result, 0) != hipSuccess)
    return 0;
  ep.result = (uint64_t *)d_result;
  ck_region(&ep, ctx->d_enc_ck, sh.ck_slots, sh.S);
  hipStream_t s = (hipStream_t)hip_stream;
  uint64_t result[kEncResultWords] = {};
  if (launch_encode(ep, ctx->geom.num_cus, s) != hipSuccess)
    return 0;
  if (hipStreamSynchronize(s) != hipSuccess)
    return 0;
  memcpy(result, ctx->h_enc_result, sizeof(result));
  if (stamps) // printed, not returned: a tuning aid only
  {
    std::vector<uint64_t> st(nb * 4);
    if (hipMemcpy(st.data(), ep.stamps, st.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
    {
      double ph[3] = {0, 0, 0};
      uint64_t lo = ~0ull, hi = 0;
      for (uint32_t b = 0; b < ep.n_blocks; b++)
      {
        for (int k = 0; k < 3; k++)
          ph[k] += (double)(st[b * 4 + k + 1] - st[b * 4 + k]);
        lo = st[b * 4] < lo ? st[b * 4] : lo;
        hi = st[b * 4 + 3] > hi ? st[b * 4 + 3] : hi;
      }
      fprintf(stderr, "[hsrans encode stamps] blocks %u  mean us: histogram %.1f  normalise+table %.1f  rANS pass %.1f   first start -> last end %.1f us\n", ep.n_blocks,
              ph[0] / ep.n_blocks / 100.0, ph[1] / ep.n_blocks / 100.0, ph[2] / ep.n_blocks / 100.0, (double)(hi - lo) / 100.0);
      for (int k = 1; k < 3; k++) // the spread over the blocks: the kernel lasts as long as its slowest block
      {
        std::vector<uint64_t> d(ep.n_blocks);
        for (uint32_t b = 0; b < ep.n_blocks; b++)
          d[b] = st[b * 4 + k + 1] - st[b * 4 + k];
        std::sort(d.begin(), d.end());
        fprintf(stderr, "[hsrans encode stamps]   %s us: min %.1f  p10 %.1f  p25 %.1f  median %.1f  p75 %.1f  p90 %.1f  max %.1f\n", k == 1 ? "normalise+table" : "rANS pass      ",
                d[0] / 100.0, d[d.size() / 10] / 100.0, d[d.size() / 4] / 100.0, d[d.size() / 2] / 100.0, d[d.size() * 3 / 4] / 100.0, d[d.size() * 9 / 10] / 100.0, d.back() / 100.0);
      }
    }
  }
  if (!enc_result_ok(result, false)) // (word 2 is the chain count)
    return 0;
  const size_t total = (size_t)result[0];
  if (out_dplan == nullptr)
    return total;

  // ---- the stream's plan, written on the device (K_plan), wrapped into a device plan ready for hsrans_decode_device ----
  PlanHeader h;
  hsrans_dplan *d = mt_plan_begin(ctx, &ep, result, &h, s);
  if (d == nullptr)
    return 0;
  if (launch_encode_plan(ep, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
  {
    hsrans_dplan_destroy(d);
    return 0;
  }
  mt_plan_adopt(d, ep, h, s);
  *out_dplan = d;
  return total;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}


size_t hsrans_encode_device_ex(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity,
                               const hsrans_hist *hist, hsrans_encode_opts *opts, void *hip_stream, hsrans_dplan **out_dplan)
try
{
  // The device twin of hsrans_encode_ex: same arguments accepted and refused (hsrans_host.cpp encode()), same stream, same plan.
  //   raw                               -> hsrans_encode_device_raw (one wavefront)
  //   mt_, fixed, independent, no index -> hsrans_encode_device (one wavefront per block)
  //   everything else                   -> the chain: k_unit_summaries (wide) -> the block walk on the host (hsrans_host.cpp
  //                                        reference_blocks / fixed_blocks, the host encoder's own code) -> k_encode_chain (one
  //                                        wavefront: the states run through every block) -> k_gather_chain (wide)
  if (out_dplan)
    *out_dplan = nullptr;
  if (opts)
    opts->plan_size = 0;
  ChainJob job;
  const ExRoute route = ctx == nullptr ? kExRefused : ex_route(container, states, bits, d_in, length, d_out, out_capacity, opts, &job);
  if (route == kExRefused)
    return 0;
  const uint32_t S = job.S, interval = job.interval;
  const uint64_t *ig = job.ig;
  const size_t n_ig = job.n_ig, block = job.block;
  const bool want_plan = job.want_plan;
  if (route == kExRaw)
    return hsrans_encode_device_raw(ctx, states, bits, d_in, length, d_out, out_capacity, hist, interval, ig, n_ig, want_plan ? opts->plan_out : nullptr,
                                    want_plan ? opts->plan_capacity : 0, want_plan ? &opts->plan_size : nullptr, hip_stream, want_plan ? out_dplan : nullptr);
  if (route == kExBlocks)
    return hsrans_encode_device(ctx, container, states, bits, d_in, length, d_out, out_capacity, (uint32_t)block, 0, hip_stream, nullptr);
  if (route == kExBlocksPlan) // the one-wave-per-block launch writes the host encoder's plan on the device (k_plan_blocks): copied back
  {
    hsrans_dplan *dp = nullptr;
    const size_t total = hsrans_encode_device(ctx, container, states, bits, d_in, length, d_out, out_capacity, (uint32_t)block, interval, hip_stream, &dp);
    if (total == 0)
      return 0;
    const size_t psize = hsrans_dplan_read_plan(dp, opts->plan_out, opts->plan_capacity);
    if (psize == 0 || out_dplan == nullptr)
      hsrans_dplan_destroy(dp);
    if (psize == 0)
      return 0;
    opts->plan_size = psize;
    if (out_dplan != nullptr)
      *out_dplan = dp;
    return total;
  }
  // (kExChain: ex_route has applied the limits of the one-wavefront pass)

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return 0;
  hipStream_t s = (hipStream_t)hip_stream;
  const bool stamps = ctx->tuning.debug_stamps;

  // ---- a./b. unit summaries on the device, the block walk (the host encoder's) on the host ----
  double summaries_us = 0, walk_us = 0;
  if (!device_block_walk(ctx, &job, s, &summaries_us, &walk_us))
    return 0;
  const auto t2 = std::chrono::steady_clock::now();
  chain_prepare(&job);
  const size_t nb = job.spans.size(), n_units = job.n_units;
  const uint32_t n_ck = job.n_ck;

  // ---- c. the chain: one wavefront, blocks back to front; then the images into place ----
  const ChainDown down = chain_down_layout(job);
  if (!encoder_buffers(ctx, job.slot_total, down.bytes + chain_up_bytes(job), chain_ck_bytes(job)))
    return 0;
  const EncParams ep = chain_params(job, ctx->d_enc_scratch, ctx->d_enc_meta, ctx->d_enc_meta + down.bytes, ctx->d_enc_ck);
  const std::vector<ChainBlock> &cb = job.cb;
  const std::vector<uint16_t> &counts = job.counts;
  const std::vector<uint32_t> &ck_list = job.ck_list;
  uint64_t result[kEncResultWords] = {};
  bool ok = hipMemcpyAsync((void *)ep.chain_blocks, cb.data(), nb * sizeof(ChainBlock), hipMemcpyHostToDevice, s) == hipSuccess &&
            hipMemcpyAsync((void *)ep.given_counts, counts.data(), nb * 512, hipMemcpyHostToDevice, s) == hipSuccess &&
            (ck_list.empty() || hipMemcpyAsync((void *)ep.ck_groups, ck_list.data(), ck_list.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess) &&
            launch_encode_chain(ep, s) == hipSuccess &&
            hipMemcpyAsync(result, ep.result, sizeof(result), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (!stream_settle(s, ok)) // (cb / counts / ck_list may be read until here)
    return 0;
  const auto t3 = std::chrono::steady_clock::now();
  if (stamps)
    fprintf(stderr, "[hsrans chain encode] blocks %zu  units %zu  summaries %.1f us  walk %.1f us  chain+gather %.1f us\n", nb, n_units,
            summaries_us, walk_us,
            std::chrono::duration<double, std::micro>(t3 - t2).count());
  // result[1] == 0 cannot happen (out_capacity >= hsrans_capacity was checked) and result[2] != 0 only if the host's filtering of the
  // listed checkpoints and the kernel disagree: internal consistency failures, not refusals — d_out may have been written by then
  if (!enc_result_ok(result, true))
    return 0;
  const size_t total = (size_t)result[0];
  if (!want_plan)
    return total;

  // ---- d. the plan: the device's block and checkpoint records through the host encoder's plan assembly ----
  std::vector<uint64_t> img_bytes(nb), img_off(nb);
  std::vector<uint32_t> blk_states(nb * S), ck_states((size_t)n_ck * S), ck_pos(n_ck);
  if (hipMemcpy(img_bytes.data(), ep.image_bytes, nb * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(img_off.data(), ep.image_off, nb * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(blk_states.data(), ep.block_states, nb * (size_t)S * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      (n_ck && (hipMemcpy(ck_states.data(), ep.ck_states, (size_t)n_ck * S * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(ck_pos.data(), ep.ck_pos, (size_t)n_ck * 4, hipMemcpyDeviceToHost) != hipSuccess)))
    return 0;
  const size_t psize = chain_plan_finish(job, total, img_bytes.data(), img_off.data(), blk_states.data(), ck_states.data(), ck_pos.data(), opts->plan_out, opts->plan_capacity);
  if (psize == 0)
    return 0;
  opts->plan_size = psize;
  if (out_dplan != nullptr && hsrans_dplan_create(ctx, opts->plan_out, psize, out_dplan) != HSRANS_OK)
    return 0;
  return total;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}


} // extern "C"
