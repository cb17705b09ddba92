// hsrans_capi_planes_gather.cpp — hsrans_decode_device_planes_gather (include/hsrans_hip.h): element ranges of a frame of byte planes.  The
// gather object (a hsrans_planes bound to its frame, ONE hsrans_gather_set over the coded planes), the workspace layout and the host-side cut
// of the merge (hsrans_planes_gather_tasks, a pure function), the argument checks, and the call: hsrans_decode_device_gather_batch of the coded
// planes' bytes into the workspace through its public entry, then one k_planes_merge_ranges launch (hsrans_planes_gather.hip) whose task list
// goes through the context's task buffer as the gathers' lists do (gather_region_*, hsrans_capi_gather.cpp).
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"

#include "hsrans_internal.h"

static_assert(sizeof(hsrans_planes_gather_task) == 32 && sizeof(PlanesGatherTask) == sizeof(hsrans_planes_gather_task) && sizeof(hsrans_range) == 24, "planes gather ABI layout");

struct hsrans_planes_gather
{
  hsrans_ctx *ctx = nullptr;
  hsrans_planes *planes = nullptr;
  const uint8_t *d_frame = nullptr;
  size_t frame_length = 0;
  hsrans_gather_set *set = nullptr; // over the coded planes, member k = plane planes->coded[k]; null when every plane is stored
  hsrans_planes_gather_info_t last{}; // the last call's part of hsrans_planes_gather_info (under ctx->lock)
};

namespace
{
constexpr uint64_t kTask = kPlanesGatherTaskElements;

bool width_ok(uint32_t W) { return W == 2 || W == 4 || W == 8; }
bool aligned16(const void *p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }
Span span_of(const void *p, size_t bytes, bool write) { return Span{(uintptr_t)p, (uintptr_t)p + bytes, write}; }

// a non-empty range's slot in every plane's region: up16(phase + length) bytes
uint64_t slot_of(const hsrans_range &g) { return ((g.offset & 15) + g.length + 15) & ~(uint64_t)15; }

// The cut of the merge (hsrans_planes_gather_tasks' body) for ranges known to lie inside the tensor: task(record) for every task in order;
// returns the sum of the slots
template <typename Task>
uint64_t cut_ranges(const hsrans_range *ranges, uint32_t count, Task &&task)
{
  uint64_t at = 0; // B_r
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_range &g = ranges[r];
    if (g.length == 0)
      continue;
    const uint64_t phase = g.offset & 15, first = g.offset - phase, stop = g.offset + g.length;
    const int64_t delta = (int64_t)(g.dst_offset - g.offset); // (modulo 2^64: the device adds it back the same way)
    for (uint64_t src = first; src < stop; src += kTask)
      task(hsrans_planes_gather_task{src, at + (src - first), delta, src == first ? (uint32_t)phase : 0, (uint32_t)(stop - src < kTask ? stop - src : kTask)});
    at += slot_of(g);
  }
  return at;
}

// whether every range lies inside `elements` and the tasks stay below 2^31 (a launch's workgroups); *tasks, *slots: what cut_ranges will give
// (false also where a total overflows)
bool measure_ranges(const hsrans_range *ranges, uint32_t count, uint64_t elements, uint64_t *tasks, uint64_t *slots)
{
  *tasks = *slots = 0;
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_range &g = ranges[r];
    if (!gather_extent_ok(g.offset, g.length, elements))
      return false;
    if (g.length == 0)
      continue;
    const uint64_t slot = slot_of(g);
    if (slot < g.length || *slots + slot < *slots)
      return false;
    *slots += slot;
    *tasks += ((g.offset & 15) + g.length + kTask - 1) / kTask;
    if (*tasks >= 0x80000000u)
      return false;
  }
  return true;
}
} // namespace

extern "C" size_t hsrans_planes_gather_workspace_bytes(uint32_t elem_size, uint32_t count, uint64_t total_elements)
{
  const uint64_t bytes = total_elements + 30 * (uint64_t)count;
  if (!width_ok(elem_size) || bytes < total_elements || bytes > (~(uint64_t)0 - 255) / elem_size)
    return 0;
  return elem_size * up256((size_t)bytes);
}

extern "C" size_t hsrans_planes_gather_tasks(const hsrans_range *ranges, uint32_t count, uint64_t elements, hsrans_planes_gather_task *out, size_t capacity)
{
  uint64_t tasks = 0, slots = 0;
  if ((ranges == nullptr && count > 0) || (out == nullptr && capacity > 0) || !measure_ranges(ranges, count, elements, &tasks, &slots))
    return 0;
  if (capacity == 0) // (the count alone: no walk over up to 2^31 tasks)
    return (size_t)tasks;
  size_t n = 0;
  cut_ranges(ranges, count, [&](const hsrans_planes_gather_task &t) {
    if (n < capacity)
      out[n] = t;
    n++;
  });
  return n;
}

extern "C" void hsrans_planes_gather_destroy(hsrans_planes_gather *pg)
{
  if (pg == nullptr)
    return;
  if (pg->set != nullptr)
    hsrans_gather_set_destroy(pg->set);
  delete pg;
}

extern "C" int hsrans_planes_gather_create(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, hsrans_planes_gather **out)
try
{
  if (out == nullptr)
    return HSRANS_E_ARG;
  *out = nullptr;
  if (ctx == nullptr || planes == nullptr || planes->ctx != ctx || !aligned16(d_frame) || frame_length < planes->desc.frame_length)
    return HSRANS_E_ARG;
  hsrans_planes_gather *pg = new (std::nothrow) hsrans_planes_gather;
  if (pg == nullptr)
    return HSRANS_E_HIP;
  pg->ctx = ctx;
  pg->planes = planes;
  pg->d_frame = (const uint8_t *)d_frame;
  pg->frame_length = frame_length;
  pg->last.coded = (uint32_t)planes->coded.size();
  pg->last.stored = planes->desc.elem_size - pg->last.coded;
  if (!planes->coded.empty())
  {
    const void *streams[HSRANS_PLANES_MAX];
    size_t lengths[HSRANS_PLANES_MAX];
    for (size_t k = 0; k < planes->coded.size(); k++)
    {
      const uint32_t p = planes->coded[k];
      streams[k] = pg->d_frame + planes->desc.offset[p];
      lengths[k] = (size_t)planes->desc.length[p];
    }
    const int rc = hsrans_gather_set_create(ctx, planes->dplans.data(), streams, lengths, (uint32_t)planes->coded.size(), &pg->set);
    if (rc != HSRANS_OK)
    {
      delete pg;
      return rc;
    }
  }
  *out = pg;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_decode_device_planes_gather(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, void *d_out, size_t out_capacity,
                                                  void *d_work, size_t work_bytes, void *hip_stream)
try
{
  if (ctx == nullptr || pg == nullptr || pg->ctx != ctx || !aligned16(d_out) || !aligned16(d_work) || (ranges == nullptr && count > 0))
    return HSRANS_E_ARG;
  const hsrans_planes &planes = *pg->planes;
  const hsrans_planes_desc &desc = planes.desc;
  const uint32_t W = desc.elem_size, coded = (uint32_t)planes.coded.size();

  // ---- everything checked before anything is launched or uploaded ----
  uint64_t n_tasks = 0, slots = 0;
  if ((uint64_t)count * W >= 0x80000000u || !measure_ranges(ranges, count, desc.elements, &n_tasks, &slots))
    return HSRANS_E_ARG;
  for (uint32_t r = 0; r < count; r++)
  {
    const uint64_t end = ranges[r].dst_offset + ranges[r].length;
    if (end < ranges[r].dst_offset || end > out_capacity / W)
      return HSRANS_E_ARG;
  }
  const size_t stride = up256((size_t)slots); // (slots <= elements + 30 count: no overflow here or below)
  if (slots > (~(uint64_t)0 - 255) / W || work_bytes < W * stride)
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans{span_of(pg->d_frame, pg->frame_length, false), span_of(d_out, out_capacity, true), span_of(d_work, work_bytes, true)};
    if (!spans_disjoint(spans))
      return HSRANS_E_ARG;
  }
  {
    std::lock_guard<std::mutex> lk(ctx->lock);
    pg->last.rows = pg->last.merge_tasks = pg->last.launches = 0;
  }
  if (n_tasks == 0)
    return HSRANS_OK;

  // ---- the coded planes' bytes into their regions: row (r, k) of the gather = range r of member k, to region coded[k] + B_r + phase ----
  uint32_t set_launches = 0;
  if (coded != 0)
  {
    std::vector<hsrans_member_range> rows((size_t)count * coded);
    uint64_t at = 0;
    for (uint32_t r = 0; r < count; r++)
    {
      const hsrans_range &g = ranges[r];
      for (uint32_t k = 0; k < coded; k++)
        rows[(size_t)r * coded + k] = hsrans_member_range{g.offset, g.length, (uint64_t)planes.coded[k] * stride + at + (g.length != 0 ? (g.offset & 15) : 0), k, 0};
      at += g.length != 0 ? slot_of(g) : 0;
    }
    // (ctx->lock is not held here: hsrans_decode_device_gather_batch takes it, and it is not recursive)
    const int rc = hsrans_decode_device_gather_batch(ctx, pg->set, rows.data(), (uint32_t)rows.size(), d_work, W * stride, hip_stream);
    if (rc != HSRANS_OK)
      return rc;
    hsrans_gather_set_info_t si{};
    if (hsrans_gather_set_info(pg->set, &si) != HSRANS_OK)
      return HSRANS_E_HIP;
    set_launches = si.launches;
  }

  // ---- the merge behind it: its task list through the context's task buffer, ordered with the context's gathers ----
  PlanePtrs src{};
  uint32_t work_mask = 0;
  for (uint32_t p = 0; p < W; p++)
  {
    const bool is_stored = (desc.stored_mask >> p) & 1;
    src.p[p] = is_stored ? (uint8_t *)pg->d_frame + desc.offset[p] : (uint8_t *)d_work + p * stride;
    work_mask |= is_stored ? 0 : 1u << p;
  }
  std::lock_guard<std::mutex> lk(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t list_bytes = (size_t)n_tasks * sizeof(PlanesGatherTask), need = up256(list_bytes);
  GatherRegion region;
  const int rc = gather_region_take(ctx, need, &region);
  if (rc != HSRANS_OK)
    return rc;
  hsrans_planes_gather_task *list = (hsrans_planes_gather_task *)region.host;
  size_t n = 0;
  cut_ranges(ranges, count, [&](const hsrans_planes_gather_task &t) { list[n++] = t; });
  if (gather_region_order(ctx, s) != HSRANS_OK)
    return HSRANS_E_HIP;
  if (hipMemcpyAsync(region.dev, region.host, list_bytes, hipMemcpyHostToDevice, s) != hipSuccess ||
      launch_planes_merge_ranges(W, src, work_mask, (const PlanesGatherTask *)region.dev, (uint32_t)n_tasks, d_out, s) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  const int rc_commit = gather_region_commit(ctx, region, s);
  if (rc_commit != HSRANS_OK)
    return rc_commit;
  pg->last.rows = count * coded;
  pg->last.merge_tasks = (uint32_t)n_tasks;
  pg->last.launches = set_launches + 1;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_gather_status(hsrans_ctx *ctx, hsrans_planes_gather *pg, void *hip_stream, int *plane_status)
try
{
  if (ctx == nullptr || pg == nullptr || pg->ctx != ctx)
    return HSRANS_E_ARG;
  const hsrans_planes &planes = *pg->planes;
  for (uint32_t p = 0; plane_status != nullptr && p < planes.desc.elem_size; p++)
    plane_status[p] = HSRANS_OK;
  if (pg->set == nullptr) // (every plane stored: nothing to report, but the call still waits for the stream as the set's does)
    return hipSetDevice(ctx->device) == hipSuccess && stream_settle((hipStream_t)hip_stream, true) ? HSRANS_OK : HSRANS_E_HIP;
  int member_status[HSRANS_PLANES_MAX] = {};
  const int rc = hsrans_gather_set_status(ctx, pg->set, hip_stream, member_status);
  for (size_t k = 0; plane_status != nullptr && k < planes.coded.size(); k++)
    plane_status[planes.coded[k]] = member_status[k];
  return rc;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_gather_info(const hsrans_planes_gather *pg, hsrans_planes_gather_info_t *info)
{
  if (pg == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  std::lock_guard<std::mutex> lk(pg->ctx->lock);
  *info = pg->last;
  return HSRANS_OK;
}
