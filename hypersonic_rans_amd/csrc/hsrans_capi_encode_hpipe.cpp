// hsrans_capi_encode_hpipe.cpp — host-resident input encoded on the GPU, PCIe legs overlapped: hsrans_encode_host_pipelined.
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h); the encode-side twin of hsrans_capi_hpipe.cpp.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_encode.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"

namespace
{
// every byte of in[0, n) equals in[0]: the block is a single-symbol block (hsrans_host.cpp fixed_blocks: one distinct symbol)
bool one_symbol(const uint8_t *in, size_t n)
{
  uint64_t w = 0x0101010101010101ull * in[0], v;
  size_t i = 0;
  for (; i + 8 <= n; i += 8)
  {
    memcpy(&v, in + i, 8);
    if (v != w)
      return false;
  }
  for (; i < n; i++)
    if (in[i] != in[0])
      return false;
  return true;
}
} // namespace

extern "C"
{

size_t hsrans_encode_host_pipelined(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out,
                                    size_t out_capacity, hsrans_encode_opts *opts, uint32_t n_slices)
try
{
  // Three legs on the context's pipe streams: slice k's input goes up while slice k-1 is encoded (hsrans_encode_device's kernels on the
  // slice's blocks, then K_scan / K_gather carrying the stream position from slice to slice: EncCarry) and slice k-2's images come down
  // from a staging ring to out + (their position in the stream), which the host reads from mapped result words after an event.  The
  // plan, when asked for, is written once after the last slice by k_plan_blocks from the block records every slice left on the device.
  if (opts)
    opts->plan_size = 0;
  EncShape sh; // (hsrans_encode_device's block rules)
  if (ctx == nullptr || opts == nullptr || container != HSRANS_MT || in == nullptr || out == nullptr || opts->flags != HSRANS_ENC_INDEPENDENT_BLOCKS ||
      opts->n_index_groups != 0 || (opts->index_interval != 0 && opts->plan_out == nullptr) ||
      !mt_shape(states, bits, length, out_capacity, opts->block_size, opts->index_interval, true, &sh))
    return 0;
  const uint32_t S = sh.S, nb = sh.n_blocks, interval = sh.interval, max_ck = sh.max_ck;
  const size_t block = sh.block;
  const bool want_plan = interval != 0;
  auto block_end = [&](uint32_t b) { return b + 1 == nb ? length : (size_t)(b + 1) * block; };
  auto chains_of = [&](uint32_t b) -> uint64_t { // a coded block's chains (encode_body: 1 + one per checkpoint)
    const uint64_t whole = (block_end(b) - (size_t)b * block) / S;
    return 1 + (whole >= 1 ? (whole - 1) / interval : 0);
  };
  if (want_plan)
  {
    // the plan's size depends on which blocks hold one symbol only (one chain each): refused here, before anything is launched, when
    // the plan cannot fit; the input is only looked at when the capacity lies between the fewest and the most chains possible
    uint64_t most = 0;
    for (uint32_t b = 0; b < nb; b++)
      most += chains_of(b);
    const uint32_t flags = mt_plan_header(S, bits, length, 0, 1).flags;
    if (most > 0xFFFFFFFFull || opts->plan_capacity < plan_size(nb, nb, S, flags))
      return 0;
    if (opts->plan_capacity < plan_size((uint32_t)most, (uint32_t)most, S, flags))
    {
      uint64_t chains = 0;
      for (uint32_t b = 0; b < nb; b++)
        chains += one_symbol(in + (size_t)b * block, block_end(b) - (size_t)b * block) ? 1 : chains_of(b);
      if (opts->plan_capacity < plan_size((uint32_t)chains, (uint32_t)chains, S, flags))
        return 0;
    }
  }
  // slices: runs of whole blocks (hsrans_hpipe_create's rule when n_slices is 0: 2..16 of >= 16 MiB)
  if (n_slices == 0)
    n_slices = (uint32_t)std::min<uint64_t>(16, std::max<uint64_t>(2, length >> 24));
  const uint32_t ns = std::min(n_slices, nb);
  std::vector<uint32_t> first(ns + 1);
  size_t in_slot = 0;
  uint32_t most_blocks = 0;
  for (uint32_t k = 0; k <= ns; k++)
    first[k] = (uint32_t)((uint64_t)nb * k / ns);
  for (uint32_t k = 0; k < ns; k++)
  {
    most_blocks = std::max(most_blocks, first[k + 1] - first[k]);
    in_slot = std::max(in_slot, block_end(first[k + 1] - 1) - (size_t)first[k] * block);
  }
  in_slot = up256(in_slot);
  const uint64_t slot_bytes = sh.slot_bytes;
  const size_t stage_slot = up256(most_blocks * slot_bytes); // (an image never outgrows its slot)
  const size_t head_bytes = 16 + 4 * (size_t)S;
  // per-block records of the whole stream (the plan reads them after the last slice), the one slice's counts, the carry, the heads
  Carve at;
  at.take((size_t)nb * 8); // image_bytes
  const size_t off_off = at.take((size_t)nb * 8), off_cc = at.take((size_t)nb * 4), off_co = at.take((size_t)nb * 4);
  const size_t off_counts = at.take((size_t)most_blocks * 1024), off_carry = at.take(256), off_heads = at.take(want_plan ? (size_t)nb * head_bytes : 0);
  const size_t meta_bytes = at.at;
  const size_t ck_slots = want_plan && max_ck ? (size_t)nb * max_ck : 1;
  constexpr uint32_t kRing = 2; // input and staging slots: slice k reuses slice k-2's once its encode / download is done

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return 0;
  {
    std::lock_guard<std::mutex> sguard(ctx->stream_lock);
    for (hipStream_t &st : ctx->pipe_streams)
      if (st == nullptr && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess)
      {
        st = nullptr;
        return 0;
      }
  }
  hipStream_t up = ctx->pipe_streams[0], enc = ctx->pipe_streams[1], down = ctx->pipe_streams[2];
  const size_t result_words = 8 + (size_t)ns * kEncResultWords; // [0, 4): the carry's start; slice k's result words at 8 + 8 k
  if (!grow(&ctx->d_in, &ctx->d_in_cap, kRing * in_slot) || !grow(&ctx->d_out, &ctx->d_out_cap, kRing * stage_slot) ||
      !encoder_buffers(ctx, most_blocks * slot_bytes, meta_bytes, ck_region_bytes(ck_slots, S)) ||
      !grow_pinned_mapped(&ctx->h_pipe_result, &ctx->h_pipe_result_cap, result_words * 8))
    return 0;
  uint64_t *h_res = (uint64_t *)ctx->h_pipe_result;
  void *d_res_v = nullptr;
  if (hipHostGetDevicePointer(&d_res_v, h_res, 0) != hipSuccess)
    return 0;
  uint64_t *d_res = (uint64_t *)d_res_v;
  uint8_t *meta = ctx->d_enc_meta;
  uint64_t *g_bytes = (uint64_t *)meta, *g_off = (uint64_t *)(meta + off_off);
  uint32_t *g_cc = (uint32_t *)(meta + off_cc), *g_co = (uint32_t *)(meta + off_co);
  EncCarry *d_carry = (EncCarry *)(meta + off_carry);
  uint8_t *g_heads = want_plan ? meta + off_heads : nullptr;
  EncParams whole{}; // (the whole stream's checkpoint region: a slice's blocks begin inside it)
  ck_region(&whole, ctx->d_enc_ck, ck_slots, S);
  uint32_t *g_ck_states = whole.ck_states, *g_ck_pos = whole.ck_pos;
  memset(h_res, 0, result_words * 8);
  h_res[0] = 16; // EncCarry{16, 0, 0, 0}: the file header comes first

  std::vector<hipEvent_t> ev(3 * (size_t)ns, nullptr); // up_done[k], enc_done[k], down_done[k]
  bool ok = true;
  for (hipEvent_t &e : ev)
    ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  auto up_done = [&](uint32_t k) { return ev[3 * (size_t)k]; };
  auto enc_done = [&](uint32_t k) { return ev[3 * (size_t)k + 1]; };
  auto down_done = [&](uint32_t k) { return ev[3 * (size_t)k + 2]; };
  ok = ok && hipMemcpyAsync(d_carry, h_res, sizeof(EncCarry), hipMemcpyHostToDevice, enc) == hipSuccess;

  uint64_t last[kEncResultWords] = {}; // the result words of the slice that came in last: the whole stream's once all are in
  // step j queues slice j's upload and encode, then (one slice behind) waits for slice j-1's result words and queues its download:
  // the upload of slice j is in flight while the host waits, and the next upload is queued before it ends
  for (uint32_t j = 0; ok && j <= ns; j++)
  {
    if (j < ns)
    {
      const uint32_t b0 = first[j], b1 = first[j + 1];
      const size_t begin = (size_t)b0 * block, len = block_end(b1 - 1) - begin;
      uint8_t *d_in = ctx->d_in + (j % kRing) * in_slot;
      ok = (j < kRing || hipStreamWaitEvent(up, enc_done(j - kRing), 0) == hipSuccess) &&
           hipMemcpyAsync(d_in, in + begin, len, hipMemcpyHostToDevice, up) == hipSuccess && hipEventRecord(up_done(j), up) == hipSuccess &&
           hipStreamWaitEvent(enc, up_done(j), 0) == hipSuccess && (j < kRing || hipStreamWaitEvent(enc, down_done(j - kRing), 0) == hipSuccess);
      EncParams ep{};
      ep.S = S;
      ep.bits = bits;
      ep.in = d_in;
      ep.n = len;
      ep.out = ctx->d_out + (j % kRing) * stage_slot;
      ep.out_cap = stage_slot;
      ep.scratch = ctx->d_enc_scratch;
      ep.slot_bytes = slot_bytes;
      ep.block = block;
      ep.n_blocks = b1 - b0;
      ep.image_bytes = g_bytes + b0;
      ep.image_off = g_off + b0;
      ep.chain_count = g_cc + b0;
      ep.chain_off = g_co + b0;
      ep.result = d_res + 8 + (size_t)j * kEncResultWords;
      ep.raw_counts = (const uint32_t *)(meta + off_counts);
      ep.interval = want_plan ? interval : 0;
      ep.max_ck = max_ck;
      ep.ck_states = g_ck_states + (want_plan && max_ck ? (size_t)b0 * max_ck * S : 0);
      ep.ck_pos = g_ck_pos + (want_plan && max_ck ? (size_t)b0 * max_ck : 0);
      ok = ok && launch_encode_slice(ep, d_carry, j + 1 == ns, g_heads ? g_heads + (size_t)b0 * head_bytes : nullptr, ctx->geom.num_cus, enc) == hipSuccess &&
           hipEventRecord(enc_done(j), enc) == hipSuccess;
    }
    if (ok && j >= 1)
    {
      const uint32_t k = j - 1;
      ok = hipEventSynchronize(enc_done(k)) == hipSuccess;
      const volatile uint64_t *r = h_res + 8 + (size_t)k * kEncResultWords;
      const uint64_t end = r[0], base = r[5];
      ok = ok && r[1] == 1 && base >= 16 && end >= base && end <= out_capacity;
      if (ok)
        std::copy(r, r + kEncResultWords, last);
      ok = ok && hipStreamWaitEvent(down, enc_done(k), 0) == hipSuccess &&
           (end == base || hipMemcpyAsync(out + base, ctx->d_out + (k % kRing) * stage_slot, end - base, hipMemcpyDeviceToHost, down) == hipSuccess) &&
           hipEventRecord(down_done(k), down) == hipSuccess;
    }
  }
  // the plan, after the last slice (its chain count is known now), on the encode stream while the last slice comes down
  PlanHeader h{};
  size_t psize = 0;
  if (ok && want_plan)
  {
    EncParams ep{};
    ep.S = S;
    ep.bits = bits;
    ep.n = length;
    ep.block = block;
    ep.n_blocks = nb;
    ep.image_bytes = g_bytes;
    ep.image_off = g_off;
    ep.chain_count = g_cc;
    ep.chain_off = g_co;
    ep.interval = interval;
    ep.max_ck = max_ck;
    ep.ck_states = g_ck_states;
    ep.ck_pos = g_ck_pos;
    ep.scratch = g_heads;
    ok = mt_result_header(ep, last, &h); // (as hsrans_encode_device's)
    psize = (size_t)plan_size(h.n_chains, h.n_pieces, S, h.flags);
    ok = ok && psize <= opts->plan_capacity && grow(&ctx->d_plan, &ctx->d_plan_cap, psize);
    if (ok)
    {
      ep.plan = ctx->d_plan;
      ep.n_chains = h.n_chains;
      ok = hipMemsetAsync(ctx->d_plan, 0, psize, enc) == hipSuccess && hipMemcpyAsync(ctx->d_plan, &h, sizeof(h), hipMemcpyHostToDevice, enc) == hipSuccess &&
           launch_encode_plan_carried(ep, enc) == hipSuccess &&
           hipMemcpyAsync(opts->plan_out, ctx->d_plan, psize, hipMemcpyDeviceToHost, enc) == hipSuccess;
    }
  }
  // whatever happened, nothing that was queued may still be reading `in` or writing `out` / the plan when this returns
  const bool s1 = hipStreamSynchronize(up) == hipSuccess, s2 = hipStreamSynchronize(enc) == hipSuccess, s3 = hipStreamSynchronize(down) == hipSuccess;
  for (hipEvent_t e : ev)
    if (e)
      (void)hipEventDestroy(e);
  if (!ok || !s1 || !s2 || !s3)
  {
    (void)hipGetLastError();
    return 0;
  }
  const uint64_t file_header[2] = {(uint64_t)length, last[0]}; // decodedLen | streamLen, once the last slice's end is known
  memcpy(out, file_header, 16);
  if (want_plan)
    opts->plan_size = psize;
  return (size_t)last[0];
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

} // extern "C"
