// hsrans_decode_device_gather (include/hsrans_hip.h): byte ranges of one stream in one launch — the host-side cut of the ranges into
// one-wave tasks (hsrans_gather_tasks, a pure function), the argument checks, the context's task buffer and the launch (k_gather,
// kernels_gather.h, through launch_gather in hsrans_kernels.hip).
// hsrans_decode_device_gather_indirect: the same for ranges that are in device memory — no cut, no task buffer and no lock here: the
// device cuts (k_gather_cut, k_gather_ranges through launch_gather_ranges), the caller brings the workspace.
// gather_region_*: the context's task buffer as regions, shared with hsrans_decode_device_gather_batch (hsrans_capi_gather_batch.cpp).
// What all three entries do alike is written once: the rules of a range (gather_range_ok, gather_range_tasks: hsrans_kernels.h, the
// device's too) and the plan test, the fill of a GatherSource and the cut of a range at multiples of L (gather_plan_ok,
// gather_source_of, gather_cut_range: hsrans_internal.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "../../include/hsrans_hip.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"

static_assert(sizeof(hsrans_range) == 24 && sizeof(hsrans_gather_task) == 24 && sizeof(GatherTask) == sizeof(hsrans_gather_task) && sizeof(GatherRange) == sizeof(hsrans_range),
              "gather ABI layout");

// The floor of a task's segment length, in decoded bytes.  A task costs its wave a prologue (chain search, start states, perhaps a table
// build, the first stream chunks) whatever its length, so segments far below a few KiB are mostly prologue; segments far above it leave
// small requests on few waves.  Measured (tools/gather_rate.py --segments, profiles/r10_gather_rate.jsonl; MI355X, 100 MB, 64 states, 11 bits, a
// checkpoint every 32 groups = 2 KiB, rotated over 4 sets, us per gather, destinations aligned / packed; a plan made under
// HSRANS_GATHER_MIN_SEGMENT gathers with that floor, Tuning::gather_min_segment):
//     floor               1 KiB         2 KiB         4 KiB         8 KiB         16 KiB
//     raw  1 % x 4 KiB    29.9 / 31.4   29.3 / 31.5   22.8 / 27.7   26.3 / 31.4   26.3 / 31.3
//     raw 10 % x 64 KiB   43.0 / 45.0   42.4 / 44.8   38.1 / 45.8   45.1 / 58.5   60.3 / 82.3
//     mt_  1 % x 4 KiB    40.8 / 44.7   44.7 / 44.0   33.7 / 39.2   37.5 / 42.8   37.3 / 42.8
//     mt_ 10 % x 64 KiB   69.2 / 77.6   69.3 / 78.2   52.0 / 60.3   59.1 / 72.1   73.1 / 95.7
// (1 and 2 KiB both give 2 KiB segments here: the floor is raised to a multiple of the checkpoint interval.)  4 KiB wins or ties every row.
static constexpr uint64_t kGatherMinSegment = 4096;

// the segment length for a floor (hsrans_gather_segment's rule)
static uint64_t segment_for(uint64_t floor, uint64_t decoded_len, uint32_t n_chains, uint32_t states, uint32_t interval)
{
  if (n_chains == 0 || states == 0)
    return 0;
  uint64_t base = (uint64_t)interval * states;
  if (base == 0)
  {
    const uint64_t mean = (decoded_len + n_chains - 1) / n_chains;
    base = (mean + states - 1) / states * states;
    if (base == 0)
      base = states;
  }
  return base >= floor ? base : base * ((floor + base - 1) / base);
}

// hsrans_gather_tasks' body for a segment length L
static size_t cut_tasks(uint64_t L, uint64_t decoded_len, const hsrans_range *ranges, uint32_t count, hsrans_gather_task *out, size_t capacity)
{
  if (L == 0 || (ranges == nullptr && count > 0) || (out == nullptr && capacity > 0))
    return 0;
  for (uint32_t r = 0; r < count; r++)
    if (!gather_extent_ok(ranges[r].offset, ranges[r].length, decoded_len))
      return 0;
  size_t n = 0;
  for (uint32_t r = 0; r < count; r++)
  {
    const int64_t delta = (int64_t)(ranges[r].dst_offset - ranges[r].offset); // (modulo 2^64: the device adds it back the same way)
    gather_cut_range(ranges[r].offset, ranges[r].length, L, [&](uint64_t b, uint64_t e) {
      if (n < capacity)
        out[n] = hsrans_gather_task{b, e, delta};
      n++;
    });
  }
  return n;
}

// the launch parameters of a gather of d over the stream at d_stream into d_dst, all but the tasks
static GatherParams gather_params_of(const hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_dst)
{
  const GatherSource gs = gather_source_of(d, d_stream, stream_length);
  GatherParams gp{};
  gp.stream = gs.stream;
  gp.stream_len = gs.stream_len;
  gp.dst = (uint8_t *)d_dst;
  gp.plan = gs.plan;
  gp.status = gs.status;
  gp.table = gs.table;
  gp.hist_copy = gs.hist_copy;
  gp.hist_off = gs.hist_off;
  return gp;
}

// (the floor: the compiled-in one unless the plan was made under HSRANS_GATHER_MIN_SEGMENT, the sweep's knob)
uint64_t gather_segment_of(const hsrans_dplan *d)
{
  const PlanHeader &h = d->hdr;
  return segment_for(d->tuning.gather_min_segment ? d->tuning.gather_min_segment : kGatherMinSegment, h.decoded_len, h.n_chains, h.states, h.interval);
}

// The task buffers — page-locked on the host, so that the copy really is asynchronous, and on the device — belong to the context and are
// used as two halves, call after call taking the next region: a queued gather's tasks are never overwritten under it.  Before a half is
// entered again the last launch that used it is waited for (a wait that only happens when the device is more than half a buffer of task
// lists behind).
int gather_region_take(hsrans_ctx *ctx, size_t need, GatherRegion *region)
{
  for (int k = 0; k < 2; k++)
    if (ctx->gather_ev[k] == nullptr && hipEventCreateWithFlags(&ctx->gather_ev[k], hipEventDisableTiming) != hipSuccess)
      return HSRANS_E_HIP;
  if (2 * need > ctx->d_gather_cap || 2 * need > ctx->h_gather_cap)
  {
    for (int k = 0; k < 2; k++) // (nothing queued may still be reading what is about to be freed)
      if (ctx->gather_ev_used[k] && hipEventSynchronize(ctx->gather_ev[k]) != hipSuccess)
        return HSRANS_E_HIP;
    const size_t want = 2 * need > (256u << 10) ? 2 * need : (256u << 10);
    if (!grow(&ctx->d_gather, &ctx->d_gather_cap, want) || !grow_pinned(&ctx->h_gather, &ctx->h_gather_cap, want))
      return HSRANS_E_HIP;
    ctx->gather_cursor = 0;
    ctx->gather_ev_used[0] = ctx->gather_ev_used[1] = false;
  }
  const size_t half = ((ctx->d_gather_cap < ctx->h_gather_cap ? ctx->d_gather_cap : ctx->h_gather_cap) / 2) & ~(size_t)255;
  uint32_t hf = ctx->gather_cursor >= half ? 1 : 0;
  if (ctx->gather_cursor - hf * half + need > half)
  {
    hf ^= 1;
    ctx->gather_cursor = hf * half;
  }
  // (a region never straddles the halves, so a half is always entered at its first byte)
  if (ctx->gather_cursor == hf * half && ctx->gather_ev_used[hf] && hipEventSynchronize(ctx->gather_ev[hf]) != hipSuccess)
    return HSRANS_E_HIP;
  region->host = ctx->h_gather + ctx->gather_cursor;
  region->dev = ctx->d_gather + ctx->gather_cursor;
  region->half = hf;
  region->bytes = need;
  return HSRANS_OK;
}

// the event of a half's last launch stands for every launch before it
int gather_region_order(hsrans_ctx *ctx, hipStream_t s)
{
  if (ctx->gather_have_last && ctx->gather_last_stream != s && hipStreamWaitEvent(s, ctx->gather_ev[ctx->gather_last_half], 0) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}

int gather_region_commit(hsrans_ctx *ctx, const GatherRegion &region, hipStream_t s)
{
  if (hipEventRecord(ctx->gather_ev[region.half], s) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  ctx->gather_ev_used[region.half] = true;
  ctx->gather_have_last = true;
  ctx->gather_last_stream = s;
  ctx->gather_last_half = region.half;
  ctx->gather_cursor += region.bytes;
  return HSRANS_OK;
}

extern "C"
{

uint64_t hsrans_gather_segment(uint64_t decoded_len, uint32_t n_chains, uint32_t states, uint32_t interval)
{
  return segment_for(kGatherMinSegment, decoded_len, n_chains, states, interval);
}

size_t hsrans_gather_tasks(uint64_t decoded_len, uint32_t n_chains, uint32_t states, uint32_t interval, const hsrans_range *ranges, uint32_t count,
                           hsrans_gather_task *out, size_t capacity)
{
  return cut_tasks(hsrans_gather_segment(decoded_len, n_chains, states, interval), decoded_len, ranges, count, out, capacity);
}

int hsrans_decode_device_gather(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, const hsrans_range *ranges, uint32_t count, void *d_dst,
                                size_t dst_capacity, void *hip_stream)
{
  if (ctx == nullptr || d == nullptr || d_stream == nullptr || d_dst == nullptr || d->ctx != ctx || (ranges == nullptr && count > 0))
    return HSRANS_E_ARG;
  if (((uintptr_t)d_stream & 15) != 0)
    return HSRANS_E_ARG;
  const PlanHeader &h = d->hdr;
  bool any = false;
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_range &g = ranges[r];
    if (!gather_range_ok(g.offset, g.length, g.dst_offset, h.decoded_len, d->out_lo, d->out_hi, dst_capacity))
      return HSRANS_E_ARG;
    any = any || g.length != 0;
  }
  if (!gather_plan_ok(d, stream_length))
    return HSRANS_E_FORMAT;
  if (!any)
    return HSRANS_OK;
  const uint64_t L = gather_segment_of(d);
  const size_t n_tasks = cut_tasks(L, h.decoded_len, ranges, count, nullptr, 0);
  if (n_tasks == 0 || n_tasks > 0x7FFFFFFFu)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;

  // The task list goes up with one stream-ordered copy in front of the launch, through a region of the context's task buffers
  std::lock_guard<std::mutex> lk(ctx->lock);
  return gather_region_upload(
      ctx, n_tasks * sizeof(GatherTask), s,
      [&](uint8_t *list) { return cut_tasks(L, h.decoded_len, ranges, count, (hsrans_gather_task *)list, n_tasks) == n_tasks ? HSRANS_OK : HSRANS_E_ARG; },
      [&](const uint8_t *d_list) {
        GatherParams gp = gather_params_of(d, d_stream, stream_length, d_dst);
        gp.tasks = (const GatherTask *)d_list;
        gp.n_tasks = (uint32_t)n_tasks;
        return launch_gather(gp, gather_shape(d->tuning, h, ctx->geom, gather_table_mode(d), gp.n_tasks), s);
      });
}

size_t hsrans_gather_workspace_bytes(uint32_t max_count)
{
  // k_gather_cut's header words, then first_task[0 .. max_count]
  return up256((size_t)kGatherWsFirst * 4 + ((size_t)max_count + 1) * 4);
}

int hsrans_decode_device_gather_indirect(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, const hsrans_range *d_ranges, const uint32_t *d_count,
                                         uint32_t max_count, void *d_dst, size_t dst_capacity, void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
  if (ctx == nullptr || d == nullptr || d_stream == nullptr || d_dst == nullptr || d_ranges == nullptr || d_workspace == nullptr || d->ctx != ctx)
    return HSRANS_E_ARG;
  if (((uintptr_t)d_stream & 15) != 0 || ((uintptr_t)d_ranges & 7) != 0 || ((uintptr_t)d_count & 3) != 0 || ((uintptr_t)d_workspace & 255) != 0 ||
      workspace_bytes < hsrans_gather_workspace_bytes(max_count))
    return HSRANS_E_ARG;
  const PlanHeader &h = d->hdr;
  if (!gather_plan_ok(d, stream_length))
    return HSRANS_E_FORMAT;
  if (max_count == 0)
    return HSRANS_OK;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;

  GatherCutParams cp{};
  cp.ranges = (const GatherRange *)d_ranges;
  cp.count = d_count;
  cp.max_count = max_count;
  cp.segment = gather_segment_of(d);
  cp.decoded_len = h.decoded_len;
  cp.out_lo = d->out_lo;
  cp.out_hi = d->out_hi;
  cp.dst_capacity = dst_capacity;
  cp.workspace = (uint32_t *)d_workspace;
  cp.status = d->d_status;
  const GatherParams gp = gather_params_of(d, d_stream, stream_length, d_dst);
  const GatherShape shape = gather_ranges_shape(d->tuning, h, ctx->geom, gather_table_mode(d), max_count, dst_capacity, cp.segment);
  if (launch_gather_ranges(gp, cp, shape, (hipStream_t)hip_stream) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  return HSRANS_OK;
}

} // extern "C"
