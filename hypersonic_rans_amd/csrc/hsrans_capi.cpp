// C ABI of libhsrans_hip.so (declared in include/hsrans_hip.h).  Nothing here decodes on the CPU: every decode entry
// ends in a launch of the gfx950 kernels in hsrans_kernels.hip and fails when no usable device exists.
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
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_cpu.h"
#include "hsrans_encode.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"
#include "hsrans_batch.h"


extern "C"
{

const char *hsrans_version(void) { return "hsrans-hip 0.1 (gfx950)"; }

// ---- host-side format functions ---------------------------------------------------------------------------------
size_t hsrans_capacity(int container, int states, size_t input_size)
{
  if (!valid_codec(container, states, 10))
    return 0;
  return capacity(container, states, input_size);
}

void hsrans_make_hist(hsrans_hist *hist, const uint8_t *data, size_t size, uint32_t bits)
{
  if (hist && data && size && bits >= 10 && bits <= 15)
    make_hist(hist, data, size, bits);
}

size_t hsrans_encode(int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out, size_t out_capacity, const hsrans_hist *hist)
try
{
  return encode(container, states, bits, in, length, out, out_capacity, hist, nullptr);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_encode_ex(int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out, size_t out_capacity,
                        const hsrans_hist *hist, hsrans_encode_opts *opts)
try
{
  if (opts)
    opts->plan_size = 0;
  return encode(container, states, bits, in, length, out, out_capacity, hist, opts);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_plan_capacity(int container, int states, size_t decoded_size, uint32_t index_interval, uint32_t block_size)
{
  if (!valid_codec(container, states, 10))
    return 0;
  return plan_capacity(container, states, decoded_size, index_interval, block_size);
}

size_t hsrans_plan_build(int container, int states, uint32_t bits, const uint8_t *stream, size_t stream_length, size_t out_capacity, uint8_t *plan_out,
                         size_t plan_capacity)
try
{
  if (plan_out == nullptr)
    return 0;
  return plan_build(container, states, bits, stream, stream_length, out_capacity, plan_out, plan_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

uint32_t hsrans_plan_chain_count(const uint8_t *plan, size_t plan_size)
{
  PlanHeader h;
  return read_header(plan, plan_size, &h) ? h.n_chains : 0;
}

uint64_t hsrans_plan_decoded_length(const uint8_t *plan, size_t plan_size)
{
  PlanHeader h;
  return read_header(plan, plan_size, &h) ? h.decoded_len : 0;
}

size_t hsrans_plan_slice(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint8_t *out, size_t out_capacity)
try
{
  if (out == nullptr)
    return 0;
  return plan_slice(plan, plan_size, first_chain, chain_count, out, out_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

int hsrans_plan_chain_range(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint64_t *begin, uint64_t *end)
{
  if (begin == nullptr || end == nullptr)
    return HSRANS_E_ARG;
  return plan_chain_range(plan, plan_size, first_chain, chain_count, begin, end) ? HSRANS_OK : HSRANS_E_FORMAT;
}

int hsrans_plan_stream_ranges(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint64_t ranges[4])
{
  if (ranges == nullptr)
    return HSRANS_E_ARG;
  return plan_stream_ranges(plan, plan_size, first_chain, chain_count, ranges) ? HSRANS_OK : HSRANS_E_FORMAT;
}

// ---- host SIMD decoders (hsrans_cpu.cpp): never reached from the GPU entries below --------------------------------------
int hsrans_cpu_level(void) { return cpu::best_level(); }

size_t hsrans_decode_cpu(int level, uint32_t threads, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint8_t *out,
                         size_t out_capacity, const uint8_t *plan, size_t plan_size)
try
{
  if (in == nullptr || out == nullptr || !valid_codec(container, states, bits))
    return 0;
  if (level < 0)
    level = cpu::best_level();
  if (threads == 0)
    threads = 1;
  if (plan == nullptr)
    return cpu::decode(level, threads, container, states, bits, in, in_length, out, out_capacity);
  PlanHeader h;
  if (!read_header(plan, plan_size, &h) || (int)h.container != container || (int)h.states != states || h.bits != bits)
    return 0;
  return cpu::exec_plan(level, threads, plan, plan_size, in, in_length, out, out_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_index_build_host(int level, uint32_t threads, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length,
                               const uint64_t *groups, size_t n_groups, uint8_t *plan_out, size_t plan_capacity)
try
{
  if (level < 0)
    level = cpu::best_level();
  return cpu::index_build(level, threads ? threads : 1, container, states, bits, in, in_length, groups, n_groups, plan_out, plan_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

// ---- GPU side ---------------------------------------------------------------------------------------------------
int hsrans_ctx_create(int device, hsrans_ctx **out_ctx)
{
  if (out_ctx == nullptr)
    return HSRANS_E_ARG;
  *out_ctx = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return HSRANS_E_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess)
    return HSRANS_E_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return HSRANS_E_HIP;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) // the code object holds gfx950 ISA only
    return HSRANS_E_NO_DEVICE;
  hsrans_ctx *ctx = new (std::nothrow) hsrans_ctx;
  if (ctx == nullptr)
    return HSRANS_E_HIP;
  ctx->device = device;
  // the marketing name needs the amdgpu.ids table, which minimal images lack: fall back to the ISA name
  snprintf(ctx->name, sizeof(ctx->name), "%s%s%s (%d CUs)", prop.name, prop.name[0] ? " " : "", prop.gcnArchName, prop.multiProcessorCount);
  if (prepare_kernels(&ctx->geom) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void **)&ctx->d_status, 64) != hipSuccess)
  {
    hsrans_ctx_destroy(ctx);
    return HSRANS_E_HIP;
  }
  // HSRANS_CALIBRATE=1: fit the one-chain-per-wave index's class lengths to this device right away (~0.5 s; for callers that cannot
  // call hsrans_ctx_calibrate themselves, e.g. the drop-in entries, which create their one context on first use)
  if (ctx->tuning.calibrate)
  {
    const int crc = hsrans_ctx_calibrate(ctx, 11, 0, nullptr); // (a failed fit leaves the compiled-in lengths in place: the context is still usable)
    if (crc != HSRANS_OK)
      fprintf(stderr, "hsrans: HSRANS_CALIBRATE=1: hsrans_ctx_calibrate failed (code %d); the compiled-in class lengths stay in use\n", crc);
  }
  *out_ctx = ctx;
  return HSRANS_OK;
}

void hsrans_ctx_destroy(hsrans_ctx *ctx)
{
  if (ctx == nullptr)
    return;
  (void)hipSetDevice(ctx->device);
  if (ctx->cached_pipe)
    hsrans_hpipe_destroy(ctx->cached_pipe);
  if (ctx->host_dplan)
    hsrans_dplan_destroy(ctx->host_dplan);
  if (ctx->host_index)
    hsrans_dplan_destroy(ctx->host_index);
  if (ctx->stream)
    (void)hipStreamDestroy(ctx->stream);
  if (ctx->d_in)
    (void)hipFree(ctx->d_in);
  if (ctx->d_out)
    (void)hipFree(ctx->d_out);
  if (ctx->d_plan)
    (void)hipFree(ctx->d_plan);
  if (ctx->d_enc_scratch)
    (void)hipFree(ctx->d_enc_scratch);
  if (ctx->d_enc_meta)
    (void)hipFree(ctx->d_enc_meta);
  if (ctx->d_enc_ck)
    (void)hipFree(ctx->d_enc_ck);
  if (ctx->d_status)
    (void)hipFree(ctx->d_status);
  if (ctx->h_pin)
    (void)hipHostFree(ctx->h_pin);
  if (ctx->h_enc_result)
    (void)hipHostFree(ctx->h_enc_result);
  if (ctx->h_pipe_result)
    (void)hipHostFree(ctx->h_pipe_result);
  if (ctx->d_gather)
    (void)hipFree(ctx->d_gather);
  if (ctx->h_gather)
    (void)hipHostFree(ctx->h_gather);
  for (hipEvent_t ev : ctx->gather_ev)
    if (ev)
      (void)hipEventDestroy(ev);
  for (hipStream_t st : ctx->pipe_streams)
    if (st)
      (void)hipStreamDestroy(st);
  delete ctx;
}

const char *hsrans_ctx_device_name(const hsrans_ctx *ctx) { return ctx ? ctx->name : ""; }

uint32_t hsrans_ctx_host_index_chains(hsrans_ctx *ctx)
{
  if (ctx == nullptr)
    return 0;
  std::lock_guard<std::mutex> guard(ctx->lock);
  return ctx->host_index ? ctx->host_index->hdr.n_chains : 0;
}

// A page-locked, device-mapped host range (hipHostMalloc / hipHostRegister): the address the GPU reaches it at, else null.
extern "C++" uint8_t *device_view_of_host(const void *ptr, size_t bytes)
{
  if (ptr == nullptr || bytes == 0)
    return nullptr;
  hipPointerAttribute_t a{}, b{};
  if (hipPointerGetAttributes(&a, ptr) != hipSuccess || hipPointerGetAttributes(&b, (const uint8_t *)ptr + bytes - 1) != hipSuccess)
  {
    (void)hipGetLastError(); // pageable memory: not an error of ours
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost || b.type != hipMemoryTypeHost || a.devicePointer == nullptr || b.devicePointer == nullptr)
    return nullptr;
  if ((const uint8_t *)b.devicePointer - (const uint8_t *)a.devicePointer != (ptrdiff_t)(bytes - 1)) // one mapping, end to end
    return nullptr;
  return (uint8_t *)a.devicePointer;
}


size_t hsrans_decode_host(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint8_t *out, size_t out_capacity,
                          const uint8_t *plan, size_t plan_size)
try
{
  if (ctx == nullptr || in == nullptr || out == nullptr || !valid_codec(container, states, bits))
    return 0;

  // A caller that loops the plain decodeFunc over one file (the reference's benchmark does: src/main.cpp:860-889) pays for the
  // missing index once: the first call's decode records checkpoints (hsrans_decode_device_indexing) and the plan it leaves is kept
  // in the context; later calls on the same bytes launch it.  "The same bytes" is checked on ALL of them: the stream is uploaded
  // anyway, a wide kernel fingerprints it there, and the decode that ran beside it only counts when the fingerprint matches.
  // (block_ streams too: the one wavefront that walks their inline headers records them, and the indexed plan is assembled on the device behind it)
  const bool cacheable = plan == nullptr && (container == HSRANS_MT || container == HSRANS_RAW || container == HSRANS_BLOCK) && in_length >= 16 &&
                         !ctx->tuning.host_index_cache_off;
  const uint64_t codec_key = (uint64_t)container | ((uint64_t)states << 8) | ((uint64_t)bits << 16) | (1ull << 32);
  if (cacheable)
  {
    std::lock_guard<std::mutex> guard(ctx->lock);
    hsrans_dplan *ix = ctx->host_index;
    // (the stream's first bytes — its header, the first block header or the histogram — are compared on the host before anything is
    // launched; the fingerprint of ALL bytes is what the result then rests on)
    if (ix != nullptr && ctx->host_index_key[0] == (uint64_t)(uintptr_t)in && ctx->host_index_key[1] == in_length && ctx->host_index_key[2] == codec_key &&
        ctx->host_index_head_len == std::min<size_t>(in_length, sizeof(ctx->host_index_head)) && memcmp(ctx->host_index_head, in, ctx->host_index_head_len) == 0 &&
        ix->hdr.decoded_len <= out_capacity && hipSetDevice(ctx->device) == hipSuccess)
    {
      const size_t n = (size_t)ix->hdr.decoded_len;
      const size_t in_pad = (in_length + 15) / 16 * 16;
      if (grow(&ctx->d_in, &ctx->d_in_cap, in_pad) && grow(&ctx->d_out, &ctx->d_out_cap, n + 16) && grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, 64))
      {
        hipStream_t s = ctx->stream;
        uint32_t status = 0xFFFFFFFF;
        uint64_t sum = 0;
        bool ok = hipMemcpyAsync(ctx->d_in, in, in_length, hipMemcpyHostToDevice, s) == hipSuccess &&
                  launch_stream_checksum(ctx->d_in, in_length, (uint64_t *)ctx->d_enc_meta, s) == hipSuccess && hipMemsetAsync(ix->d_status, 0, 4, s) == hipSuccess &&
                  dplan_launch(ix, ctx->d_in, in_length, ctx->d_out, n, s) == HSRANS_OK && hipMemcpyAsync(out, ctx->d_out, n, hipMemcpyDeviceToHost, s) == hipSuccess &&
                  hipMemcpyAsync(&sum, ctx->d_enc_meta, 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
                  hipMemcpyAsync(&status, ix->d_status, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = (hipStreamSynchronize(s) == hipSuccess) && ok;
        if (ok && status == 0 && sum == ctx->host_index_key[3])
          return n;
        (void)hipGetLastError();
      }
      // other bytes at that address (or a failure): the index is dropped and the call starts over below (`out` is rewritten in full)
      hsrans_dplan_destroy(ctx->host_index);
      ctx->host_index = nullptr;
    }
  }

  std::vector<uint8_t> own_plan;
  if (plan == nullptr)
  {
    // header-only peek to size the plan, then the real planner (which repeats the reference's entry checks)
    if (in_length < 16)
      return 0;
    uint64_t out_len;
    memcpy(&out_len, in, 8);
    if (out_len > out_capacity)
      return 0;
    if (!plan_build_vec(container, states, bits, in, in_length, out_capacity, &own_plan)) // sized by the stream's own chain count
      return 0;
    plan = own_plan.data();
    plan_size = own_plan.size();
  }
  PlanHeader h;
  if (!read_header(plan, plan_size, &h) || (int)h.container != container || (int)h.states != states || h.bits != bits)
    return 0;
  if (!plan_validate(plan, plan_size, in_length, out_capacity))
    return 0;

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return 0;
  const size_t in_pad = (in_length + 15) / 16 * 16;
  // (Storing straight into a page-locked `out`, as hsrans_hpipe_decode does, was measured here too: with nothing to overlap it
  // only replaces a download copy at 55 GB/s by the kernel's own PCIe writes at 47 — 100 MB: 3.58 instead of 3.26 ms — so this
  // one-shot entry stages its output and copies it down (the knob that switched the direct stores on here is gone: settled).)
  uint8_t *out_view = nullptr;
  if (!grow(&ctx->d_in, &ctx->d_in_cap, in_pad) || (out_view == nullptr && !grow(&ctx->d_out, &ctx->d_out_cap, (size_t)h.decoded_len + 16)))
    return 0;
  hipStream_t s = ctx->stream;
  if (ctx->host_dplan == nullptr)
  {
    ctx->host_dplan = dplan_new(ctx);
    if (ctx->host_dplan == nullptr)
      return 0;
  }
  hsrans_dplan *d = ctx->host_dplan;
  // the same launch the device entry gets for this plan (persistent / direct / grouped), on the context's staging buffers
  uint32_t status = 0xFFFFFFFF;
  bool ok = hipMemcpyAsync(ctx->d_in, in, in_length, hipMemcpyHostToDevice, s) == hipSuccess && dplan_fill(d, plan, plan_size, h, s) == HSRANS_OK &&
            hipMemsetAsync(d->d_status, 0, 4, s) == hipSuccess;
  // the first decode of a stream without an index records one for the next call (see the top of the function); streams whose base
  // plan has a single short chain, or any failure of the recording path, take the plain launch
  bool indexed_now = false;
  uint64_t sum = 0;
  if (ok && cacheable && out_view == nullptr && h.interval == 0 && h.decoded_len >= (1u << 20) && grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, 64))
  {
    if (ctx->host_index)
      hsrans_dplan_destroy(ctx->host_index);
    ctx->host_index = nullptr;
    d->hdr = h;
    d->plan_bytes = plan_size;
    hsrans_dplan *ix = nullptr;
    bool have_index = launch_stream_checksum(ctx->d_in, in_length, (uint64_t *)ctx->d_enc_meta, s) == hipSuccess &&
                      hipMemcpyAsync(&sum, ctx->d_enc_meta, 8, hipMemcpyDeviceToHost, s) == hipSuccess;
    // HSRANS_HIP_STRICT=1: nothing of a `*_decode_hip_N` call runs on a host core — the raw stream's checkpoints are recorded by the one
    // wavefront that decodes it (hsrans_decode_device_indexing: ~125 ms for 100 MB, once) instead of by the host SIMD decoder's pass (~35 ms)
    if (have_index && container == HSRANS_RAW && !ctx->tuning.hip_strict)
    try
    {
      // a raw stream is ONE chain: the pass that records its checkpoints is the host SIMD decoder's (2-4 GB/s on one core, while the
      // upload is on its way; one wavefront would need four times as long), at the one-chain-per-wavefront boundaries of this device;
      // the decode itself is the indexed GPU launch
      std::vector<uint64_t> groups(2 * 8192 + 64);
      const size_t ng = hsrans_index_boundaries(ctx, states, bits, (size_t)h.decoded_len, groups.data(), groups.size());
      std::vector<uint8_t> iplan(ng ? plan_capacity_chains(HSRANS_RAW, states, (size_t)h.decoded_len, ng, 0) : 0);
      const size_t plen = ng ? cpu::index_build(cpu::best_level(), 1, HSRANS_RAW, states, bits, in, in_length, groups.data(), ng, iplan.data(), iplan.size()) : 0;
      have_index = plen != 0 && hsrans_dplan_create(ctx, iplan.data(), plen, &ix) == HSRANS_OK;
      if (have_index)
      {
        have_index = hipMemsetAsync(ix->d_status, 0, 4, s) == hipSuccess && dplan_launch(ix, ctx->d_in, in_length, ctx->d_out, (size_t)h.decoded_len, s) == HSRANS_OK &&
                     hipMemcpyAsync(&status, ix->d_status, 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess && status == 0;
        status = 0xFFFFFFFF; // (the entry's own status word is read below)
        if (!have_index)
        {
          (void)hipStreamSynchronize(s);
          hsrans_dplan_destroy(ix);
          ix = nullptr;
        }
      }
    }
    catch (...) // (bad_alloc from the vectors above: the upload of `in` and the fingerprint's copy are already queued — nothing queued
    {           // may still read `in` or write this frame when the function returns)
      (void)hipStreamSynchronize(s);
      if (ix != nullptr)
        hsrans_dplan_destroy(ix);
      return 0;
    }
    else if (have_index)
      have_index = decode_device_indexing_impl(ctx, d, ctx->d_in, in_length, ctx->d_out, (size_t)h.decoded_len, 64, s, &ix, true) == HSRANS_OK;
    if (have_index)
    {
      indexed_now = true; // (the recording pass has decoded into d_out and was synchronised: `sum` has arrived too)
      ctx->host_index = ix;
      ctx->host_index_key[0] = (uint64_t)(uintptr_t)in;
      ctx->host_index_key[1] = in_length;
      ctx->host_index_key[2] = codec_key;
      ctx->host_index_key[3] = sum;
      ctx->host_index_head_len = (uint32_t)std::min<size_t>(in_length, sizeof(ctx->host_index_head));
      memcpy(ctx->host_index_head, in, ctx->host_index_head_len);
    }
    else
      (void)hipGetLastError();
  }
  if (!indexed_now)
    ok = ok && dplan_launch(d, ctx->d_in, in_length, out_view ? out_view : ctx->d_out, (size_t)h.decoded_len, s) == HSRANS_OK;
  if (ok && out_view == nullptr)
    ok = hipMemcpyAsync(out, ctx->d_out, (size_t)h.decoded_len, hipMemcpyDeviceToHost, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(&status, d->d_status, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
  // nothing queued may still read `in` / `own_plan` or write `out` when this returns, whether or not a call above failed
  ok = (hipStreamSynchronize(s) == hipSuccess) && ok;
  return ok && status == 0 ? (size_t)h.decoded_len : 0;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_debug_read_stamps(hsrans_dplan *d, uint64_t *out, size_t capacity_u64)
{
  if (d == nullptr || d->d_stamps == nullptr || out == nullptr)
    return 0;
  const size_t n = capacity_u64 < kStampWaves * 8 ? capacity_u64 : kStampWaves * 8;
  return hipMemcpy(out, d->d_stamps, n * 8, hipMemcpyDeviceToHost) == hipSuccess ? n : 0;
}

int hsrans_decode_device(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity, void *hip_stream)
{
  if (ctx == nullptr || d == nullptr || d_stream == nullptr || d_out == nullptr || d->ctx != ctx)
    return HSRANS_E_ARG;
  if (((uintptr_t)d_stream & 15) != 0 || ((uintptr_t)d_out & 3) != 0)
    return HSRANS_E_ARG;
  if (stream_length < d->hdr.stream_len || out_capacity < d->hdr.decoded_len)
    return HSRANS_E_FORMAT;
  if (hipSetDevice(ctx->device) != hipSuccess) // the launch goes to the context's device whatever the caller's current device is
    return HSRANS_E_HIP;
  // the status word is sticky: kernels only ever OR error bits into it and hsrans_dplan_status() clears it after
  // reporting, so the launch path is exactly one kernel node (no memset node in front of it)
  return dplan_launch(d, d_stream, stream_length, d_out, out_capacity, (hipStream_t)hip_stream);
}

// the general launch: stream bytes [window_offset, +window_length) at d_window, output bytes [out_offset, +out_length) at d_out
extern "C++" int dplan_launch_ranges(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_window, size_t window_offset, size_t window_length, void *d_out, size_t out_offset,
                                     size_t out_length, void *hip_stream, const PartArgs *part_words)
{
  if (ctx == nullptr || d == nullptr || d_window == nullptr || d_out == nullptr || d->ctx != ctx)
    return HSRANS_E_ARG;
  if (((uintptr_t)d_window & 15) != 0 || (window_offset & 15) != 0 || ((uintptr_t)d_out & 3) != 0 || (out_offset & 3) != 0 ||
      (uintptr_t)d_window < window_offset || (uintptr_t)d_out < out_offset)
    return HSRANS_E_ARG;
  if (window_offset > d->hdr.stream_len || out_offset > d->hdr.decoded_len)
    return HSRANS_E_FORMAT;
  // Every byte the plan's chains read or write must be inside what the caller holds.  Lower edges: from the plan (dplan_fill
  // recorded them).  Upper edge of the stream: the kernels' buffer descriptors end at min(window end, chain's last word), so a
  // request past the window is dropped by the hardware; upper edge of the output: checked here.
  if (window_offset > d->body_lo || d->out_lo < out_offset || d->out_hi - out_offset > out_length)
    return HSRANS_E_FORMAT;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  const uint64_t end = std::min<uint64_t>((uint64_t)window_offset + window_length, d->hdr.stream_len);
  // (the kernels' own bound on the output is the end of the caller's window, not of the whole output: a path that rounded a store
  // up past a chain's end must not reach past a rank's smaller buffer either)
  const uint64_t out_end = std::min<uint64_t>((uint64_t)out_offset + out_length, d->hdr.decoded_len);
  return dplan_launch(d, (const uint8_t *)d_window - window_offset, (size_t)end, (uint8_t *)d_out - out_offset, (size_t)out_end, (hipStream_t)hip_stream, window_offset, part_words);
}

int hsrans_decode_device_window(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_window, size_t window_offset, size_t window_length, void *d_out,
                                size_t out_capacity, void *hip_stream)
{
  if (d == nullptr || out_capacity < d->hdr.decoded_len)
    return d == nullptr ? HSRANS_E_ARG : HSRANS_E_FORMAT;
  return dplan_launch_ranges(ctx, d, d_window, window_offset, window_length, d_out, 0, out_capacity, hip_stream, nullptr);
}

int hsrans_decode_device_ranges(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_window, size_t window_offset, size_t window_length, void *d_out_window,
                                size_t out_offset, size_t out_length, void *hip_stream)
{
  return dplan_launch_ranges(ctx, d, d_window, window_offset, window_length, d_out_window, out_offset, out_length, hip_stream, nullptr);
}

int hsrans_dplan_status(hsrans_ctx *ctx, hsrans_dplan *d, void *hip_stream)
{
  if (ctx == nullptr || d == nullptr)
    return HSRANS_E_ARG;
  uint32_t status = 0xFFFFFFFF;
  hipStream_t s = (hipStream_t)hip_stream;
  if (hipMemcpyAsync(&status, d->d_status, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  if (status == 0)
    return HSRANS_OK;
  if (hipMemsetAsync(d->d_status, 0, 4, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_E_DEVICE;
}

static void export_launch_info(const LaunchInfo &in, hsrans_launch_info *info)
{
  info->grid = in.grid;
  info->block = in.block;
  info->lds_bytes = in.lds_bytes;
  info->waves_per_block = in.waves_per_block;
  info->chains = in.chains;
  info->shared_table = in.shared_table;
  info->walk = in.walk;
  info->two_level = in.two_level;
  info->table_mode = in.table_mode;
  info->chains_per_wave = in.chains_per_wave;
  for (int k = 0; k < 8; k++)
    info->class_weights[k] = in.class_weights[k];
  info->dynamic_groups = in.dynamic_groups;
  info->spread = in.spread;
}

int hsrans_dplan_launch_info(const hsrans_dplan *d, hsrans_launch_info *info)
{
  if (d == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  export_launch_info(d->info, info);
  return HSRANS_OK;
}

int hsrans_launch_choice(const hsrans_ctx *ctx, const hsrans_plan_kind *plan, const hsrans_launch_facts *facts, hsrans_launch_info *info, char *kernel_name, size_t name_capacity)
{
  if (plan == nullptr || facts == nullptr || info == nullptr || kernel_name == nullptr || !valid_codec((int)plan->container, (int)plan->states, plan->bits))
    return -1;
  const DeviceGeom dg = ctx ? ctx->geom : default_geom();
  const Tuning tn = ctx ? ctx->tuning : read_tuning();
  PlanHeader h{};
  h.container = plan->container, h.states = plan->states, h.bits = plan->bits, h.flags = plan->flags;
  h.decoded_len = plan->decoded_len;
  h.n_chains = plan->n_chains, h.n_pieces = plan->n_pieces, h.shared_hist = plan->shared_hist, h.interval = plan->interval;
  LaunchFacts f;
  f.persistent = facts->persistent != 0;
  f.table_mode = facts->table_mode;
  f.interval = plan->interval;
  f.dual = facts->dual != 0;
  f.n_groups = facts->n_groups;
  f.groups_lean = facts->groups_lean != 0;
  f.spread_min_block = facts->spread_min_block;
  f.index_pass = facts->index_pass != 0;
  f.single_valid = facts->single_valid != 0;
  f.single_ring_entries = facts->single_ring_entries;
  f.calibrating = facts->calibrating != 0;
  f.tickets = facts->tickets != 0;
  f.parts = facts->parts != 0;
  f.n_parts = facts->n_parts;
  f.dealt = facts->dealt != 0;
  if (f.dealt) // (the class weights dplan_launch deals such a plan with)
    dealt_weights_now(tn, dg, plan->decoded_len / 64 / ((uint64_t)spread_grid(dg) * 16), plan->bits, f.dealt_weights);
  const LaunchChoice c = choose_launch(tn, h, dg, f);
  if (c.error != hipSuccess)
    return c.error == hipErrorNotSupported ? 1 : 2;
  export_launch_info(launch_info_of(c, h.n_chains), info);
  snprintf(kernel_name, name_capacity, "%s", hsrans::kernel_name(c.kernel));
  return 0;
}

int hsrans_dealt_shares(const hsrans_ctx *ctx, uint32_t bits, const uint32_t *block_begin, uint32_t n_blocks, uint32_t n_chains, uint64_t total_groups,
                        uint32_t *begin_out, uint16_t *split_out)
try
{
  if (block_begin == nullptr || begin_out == nullptr || split_out == nullptr || n_blocks == 0 || bits < 10 || bits > 15)
    return -1;
  for (uint32_t k = 0; k < n_blocks; k++)
    if (block_begin[k] >= block_begin[k + 1])
      return -1;
  DealtTable dt{};
  uint32_t w8[8];
  const DeviceGeom dg = ctx ? ctx->geom : default_geom();
  const Tuning tn = ctx ? ctx->tuning : read_tuning();
  const bool ok = deal_shares(tn, dg, block_begin, n_blocks, n_chains, total_groups, bits, &dt, w8);
  memcpy(begin_out, dt.begin, sizeof(dt.begin));
  memcpy(split_out, dt.split, sizeof(dt.split));
  return ok ? 1 : 0;
}
catch (...)
{
  return -1;
}

int hsrans_host_register(hsrans_ctx *ctx, void *ptr, size_t bytes)
{
  if (ctx == nullptr || ptr == nullptr || bytes == 0)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? HSRANS_OK : HSRANS_E_HIP;
}

int hsrans_host_unregister(hsrans_ctx *ctx, void *ptr)
{
  if (ctx == nullptr || ptr == nullptr)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  return hipHostUnregister(ptr) == hipSuccess ? HSRANS_OK : HSRANS_E_HIP;
}

size_t hsrans_index_boundaries(const hsrans_ctx *ctx, int states, uint32_t bits, size_t decoded_size, uint64_t *groups_out, size_t capacity)
{
  if ((states != 32 && states != 64) || bits < 10 || bits > 15 || groups_out == nullptr)
    return 0;
  const DeviceGeom dg = ctx ? ctx->geom : default_geom();
  const Tuning tn = ctx ? ctx->tuning : read_tuning();
  const uint64_t S = (uint64_t)states;
  const uint64_t T = decoded_size + 1 >= S ? (decoded_size - S + 1 + S - 1) / S : 0; // whole groups (rANS32x64_16w.cpp:223)
  const size_t chains = direct_boundaries(tn, dg, (uint32_t)states, bits, T, groups_out, capacity);
  return chains > 1 ? chains - 1 : 0;
}

size_t hsrans_plan_thin(const uint8_t *plan, size_t plan_size, const uint64_t *groups, size_t n_groups, uint8_t *out, size_t out_capacity)
try
{
  return plan_thin(plan, plan_size, groups, n_groups, out, out_capacity);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return 0;
}

size_t hsrans_plan_capacity_chains(int container, int states, size_t decoded_size, size_t extra_chains, uint32_t block_size)
{
  if (!valid_codec(container, states, 10))
    return 0;
  return plan_capacity_chains(container, states, decoded_size, extra_chains, block_size);
}

} // extern "C"
