// hsrans_capi_planes_gather.cpp — hsrans_decode_device_planes_gather (include/hsrans_hip.h): element ranges of a frame of byte planes.  The
// gather object (a hsrans_planes bound to its frame, ONE hsrans_gather_set over the coded planes), the workspace layout and the host-side cut
// of the merge (hsrans_planes_gather_tasks, a pure function), the argument checks, and the call: hsrans_decode_device_gather_batch of the coded
// planes' bytes into the workspace through its public entry, then one k_planes_merge_ranges launch (hsrans_planes_gather.hip) whose task list
// goes through the context's task buffer as the gathers' lists do (gather_region_*, hsrans_capi_gather.cpp).  The call's body is
// planes_gather_flow (hsrans_internal.h), which hsrans_capi_planes_delta.cpp runs with a base: then the merge is k_planes_merge_ranges_delta.
// hsrans_decode_device_planes_gather_indirect, at the end of the file: the same for ranges in device memory — the device cuts
// (hsrans_planes_gather_indirect.hip), by the rules of planes_cut.h that the host's cut above uses too; its body is
// planes_gather_indirect_flow, which hsrans_decode_device_planes_gather_indirect_delta runs with a base: then the merge is
// k_planes_merge_indirect_delta (hsrans_planes_gather_delta.hip).
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"
#include "planes_cut_batch.h"

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
  uint32_t *d_refused = nullptr; // the object's own status word (kStatusBadRange: k_planes_cut refused an indirect call); no plan's word is involved
};

namespace
{
static_assert(kPlanesCutTask == kPlanesGatherTaskElements, "planes_cut.h cuts at the merge kernels' task length");

// a range's slot in every plane's region (planes_cut.h: up16(phase + length) bytes, none for an empty range)
uint64_t slot_of(const hsrans_range &g) { return planes_range_slot(g.offset, g.length); }

// The cut of the merge (hsrans_planes_gather_tasks' body) for ranges known to lie inside the tensor: task(record) for every task in order;
// returns the sum of the slots.  Slot, task count and task k of a range are planes_cut.h's, which the device's cut uses as they stand.
template <typename Task>
uint64_t cut_ranges(const hsrans_range *ranges, uint32_t count, Task &&task)
{
  uint64_t at = 0; // B_r
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_range &g = ranges[r];
    for (uint64_t k = 0, n = planes_range_tasks(g.offset, g.length); k < n; k++)
      task(planes_task_at<hsrans_planes_gather_task>(g.offset, g.length, g.dst_offset, at, k));
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
    if (!planes_source_ok(g.offset, g.length, elements))
      return false;
    const uint64_t slot = slot_of(g);
    if (*slots + slot < *slots)
      return false;
    *slots += slot;
    *tasks += planes_range_tasks(g.offset, g.length);
    if (*tasks >= kPlanesCutLimit)
      return false;
  }
  return true;
}

// what the merges read plane p from: the stored plane in the frame, or region p of the workspace (p * stride), whose bit of *work_mask is set
PlanePtrs merge_sources(const hsrans_planes_desc &desc, const uint8_t *d_frame, void *d_work, size_t stride, uint32_t *work_mask)
{
  PlanePtrs src{};
  *work_mask = 0;
  for (uint32_t p = 0; p < desc.elem_size; p++)
  {
    const bool is_stored = (desc.stored_mask >> p) & 1;
    src.p[p] = is_stored ? (uint8_t *)d_frame + desc.offset[p] : (uint8_t *)d_work + p * stride;
    *work_mask |= is_stored ? 0 : 1u << p;
  }
  return src;
}
} // namespace

extern "C" size_t hsrans_planes_gather_workspace_bytes(uint32_t elem_size, uint32_t count, uint64_t total_elements)
{
  const uint64_t bytes = total_elements + 30 * (uint64_t)count;
  if (!planes_width_ok(elem_size) || bytes < total_elements || bytes > (~(uint64_t)0 - 255) / elem_size)
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
  if (pg->d_refused != nullptr)
    (void)hipFree(pg->d_refused);
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
  // the word hsrans_decode_device_planes_gather_indirect's cut reports a refusal in (as hsrans_gather_set_create makes the set's)
  if (refusal_word_create(ctx, &pg->d_refused) != HSRANS_OK)
  {
    hsrans_planes_gather_destroy(pg);
    return HSRANS_E_HIP;
  }
  *out = pg;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

int planes_gather_flow(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const PlanesBase &base, void *d_out, size_t out_capacity,
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
    if (!planes_base_spans(base, W, (size_t)desc.elements, nullptr, 0, &spans) || !spans_disjoint(spans) ||
        planes_base_meets_frame(base, pg->d_frame, pg->frame_length))
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
  uint32_t work_mask = 0;
  const PlanePtrs src = merge_sources(desc, pg->d_frame, d_work, stride, &work_mask);
  std::lock_guard<std::mutex> lk(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int rc = gather_region_upload(
      ctx, (size_t)n_tasks * sizeof(PlanesGatherTask), s,
      [&](uint8_t *host) {
        hsrans_planes_gather_task *list = (hsrans_planes_gather_task *)host;
        cut_ranges(ranges, count, [&](const hsrans_planes_gather_task &t) { *list++ = t; });
        return HSRANS_OK;
      },
      [&](const uint8_t *dev) {
        return launch_planes_merge_ranges(W, src, work_mask, (const PlanesGatherTask *)dev, (uint32_t)n_tasks, base.on ? base.d : nullptr, base.rule, d_out, s);
      });
  if (rc != HSRANS_OK)
    return rc;
  pg->last.rows = count * coded;
  pg->last.merge_tasks = (uint32_t)n_tasks;
  pg->last.launches = set_launches + 1;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_decode_device_planes_gather(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, void *d_out, size_t out_capacity,
                                                  void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_gather_flow(ctx, pg, ranges, count, PlanesBase{}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_gather_delta(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const void *d_base,
                                                        size_t base_bytes, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_gather_flow(ctx, pg, ranges, count, PlanesBase{true, d_base, base_bytes}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

// the delta entry under the other residue rule: the merge is k_planes_merge_ranges_diff (hsrans_planes_base.hip)
extern "C" int hsrans_decode_device_planes_gather_diff(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const void *d_base,
                                                       size_t base_bytes, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_gather_flow(ctx, pg, ranges, count, PlanesBase{true, d_base, base_bytes, PlanesRule::kDiff}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_planes_gather_status(hsrans_ctx *ctx, hsrans_planes_gather *pg, void *hip_stream, int *plane_status)
try
{
  if (ctx == nullptr || pg == nullptr || pg->ctx != ctx)
    return HSRANS_E_ARG;
  const hsrans_planes &planes = *pg->planes;
  for (uint32_t p = 0; plane_status != nullptr && p < planes.desc.elem_size; p++)
    plane_status[p] = HSRANS_OK;
  if (pg->set == nullptr)
    return planes_all_stored_status(ctx, hip_stream);
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

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_planes_gather_indirect: the ranges are in device memory.  Nothing of the above is cut here: k_planes_cut checks the
// ranges, lays out their slots and writes the set's rows, the set's indirect entry gathers the coded planes' bytes, k_planes_merge_indirect
// derives its tasks from what the cut left (hsrans_planes_gather_indirect.hip).  No lock, no task buffer, no allocation: kernels and
// nothing else.
// ---------------------------------------------------------------------------------------------------------------
namespace
{
static_assert(sizeof(PlanesRange) == sizeof(hsrans_range) && sizeof(PlanesSetRow) == sizeof(hsrans_member_range), "the device's view of the ranges and rows");

// the regions' distance, host-known: up256(max_elements + 30 max_count); false where hsrans_planes_gather_workspace_bytes gives 0 or the
// sum reaches 2^48 (beyond any device's memory; below it no sum of slots in k_planes_cut can wrap)
bool indirect_stride(uint32_t W, uint32_t max_count, uint64_t max_elements, size_t *stride)
{
  const uint64_t bytes = max_elements + 30 * (uint64_t)max_count;
  if (hsrans_planes_gather_workspace_bytes(W, max_count, max_elements) == 0 || bytes >= ((uint64_t)1 << 48))
    return false;
  *stride = up256((size_t)bytes);
  return true;
}

// What one indirect call launches, from what the host knows: the entry and hsrans_planes_gather_indirect_info both go through here.
struct IndirectShape
{
  uint32_t coded, set_rows, merge_grid, set_launches, launches;
};
bool indirect_shape(const hsrans_planes_gather *pg, uint32_t max_count, size_t stride, IndirectShape *shape)
{
  const uint32_t W = pg->planes->desc.elem_size;
  *shape = IndirectShape{};
  shape->coded = (uint32_t)pg->planes->coded.size();
  shape->set_rows = max_count * shape->coded; // (max_count * W < 2^31)
  if (max_count == 0)
    return true;
  shape->merge_grid = planes_merge_indirect_grid(pg->ctx->geom.num_cus, W, max_count, stride);
  if (pg->set != nullptr)
  {
    hsrans_gather_set_info_t si{};
    if (hsrans_gather_set_indirect_info(pg->set, shape->set_rows, W * stride, &si) != HSRANS_OK)
      return false;
    shape->set_launches = si.launches + 1; // (+ the set's cut)
  }
  shape->launches = shape->set_launches + 2; // (+ k_planes_cut and the merge)
  return true;
}
} // namespace

extern "C" size_t hsrans_planes_gather_indirect_workspace_bytes(uint32_t elem_size, uint32_t max_count)
{
  if (!planes_width_ok(elem_size) || (uint64_t)max_count * elem_size >= 0x80000000u)
    return 0;
  const size_t set_bytes = hsrans_gather_batch_workspace_bytes(elem_size, max_count * elem_size); // (sized for all planes coded: it needs no object)
  return set_bytes == 0 ? 0 : planes_cut_ws(elem_size, max_count).set + up256(set_bytes);
}

extern "C" int hsrans_planes_gather_indirect_info(const hsrans_planes_gather *pg, uint32_t max_count, uint64_t max_elements, size_t out_capacity,
                                                  hsrans_planes_gather_indirect_info_t *info)
try
{
  if (pg == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  const uint32_t W = pg->planes->desc.elem_size;
  size_t stride = 0;
  IndirectShape shape{};
  if (hsrans_planes_gather_indirect_workspace_bytes(W, max_count) == 0 || !indirect_stride(W, max_count, max_elements, &stride) || !indirect_shape(pg, max_count, stride, &shape))
    return HSRANS_E_ARG;
  (void)out_capacity; // (it bounds the destinations on the device; no launch is shaped by it)
  *info = hsrans_planes_gather_indirect_info_t{shape.coded, W - shape.coded, shape.set_rows, shape.merge_grid, shape.launches, shape.set_launches};
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

// the entry's whole body, and with a base hsrans_decode_device_planes_gather_indirect_delta's: the base joins the overlap rule as a read span
// that keeps clear of the frame, the ranges and the count word too, and the merge is k_planes_merge_indirect_delta on its own grid
int planes_gather_indirect_flow(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges, const uint32_t *d_count, uint32_t max_count, uint64_t max_elements,
                                const PlanesBase &base, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes,
                                void *hip_stream)
try
{
  if (ctx == nullptr || pg == nullptr || pg->ctx != ctx || d_ranges == nullptr || d_workspace == nullptr || !aligned16(d_out) || !aligned16(d_work))
    return HSRANS_E_ARG;
  if (((uintptr_t)d_ranges & 7) != 0 || ((uintptr_t)d_count & 3) != 0 || ((uintptr_t)d_workspace & 255) != 0)
    return HSRANS_E_ARG;
  const hsrans_planes &planes = *pg->planes;
  const hsrans_planes_desc &desc = planes.desc;
  const uint32_t W = desc.elem_size;
  const size_t need_ws = hsrans_planes_gather_indirect_workspace_bytes(W, max_count), need_work = hsrans_planes_gather_workspace_bytes(W, max_count, max_elements);
  size_t stride = 0;
  if (need_ws == 0 || need_work == 0 || workspace_bytes < need_ws || work_bytes < need_work || !indirect_stride(W, max_count, max_elements, &stride))
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans{span_of(pg->d_frame, pg->frame_length, false), span_of(d_ranges, (size_t)max_count * sizeof(hsrans_range), false),
                            span_of(d_out, out_capacity, true),            span_of(d_work, work_bytes, true),
                            span_of(d_workspace, workspace_bytes, true)};
    if (d_count != nullptr)
      spans.push_back(span_of(d_count, sizeof(uint32_t), false));
    std::vector<Span> inputs; // (what a base may not meet although it is only read, as the base is)
    if (base.on)
      inputs = spans;
    if (!planes_base_spans(base, W, (size_t)desc.elements, nullptr, 0, &spans) || !spans_disjoint(spans))
      return HSRANS_E_ARG;
    if (base.on && spans_meet({span_of(base.d, base.bytes, false)}, inputs)) // (the written ones among them have been refused above)
      return HSRANS_E_ARG;
  }
  if (max_count == 0)
    return HSRANS_OK;
  IndirectShape shape{};
  if (!indirect_shape(pg, max_count, stride, &shape))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;

  // ---- the cut: slots, task prefix and the set's rows into the control workspace ----
  const PlanesCutWs ws = planes_cut_ws(W, max_count);
  uint8_t *const control = (uint8_t *)d_workspace;
  PlanesCutParams cp{};
  cp.ranges = (const PlanesRange *)d_ranges;
  cp.count = d_count;
  cp.max_count = max_count;
  cp.coded = shape.coded;
  for (uint32_t k = 0; k < shape.coded; k++)
    cp.coded_planes |= planes.coded[k] << (4 * k);
  cp.elements = desc.elements;
  cp.out_elements = out_capacity / W;
  cp.stride = stride;
  cp.header = (uint32_t *)control;
  cp.first_task = (uint32_t *)(control + ws.first_task);
  cp.base = (uint64_t *)(control + ws.base);
  cp.rows = (PlanesSetRow *)(control + ws.rows);
  cp.status = pg->d_refused;
  if (launch_planes_cut(cp, s) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }

  // ---- the coded planes' bytes into their regions, through the set's public entry as the host-ranges call goes through the batch entry ----
  if (pg->set != nullptr)
  {
    const int rc = hsrans_decode_device_gather_batch_indirect(ctx, pg->set, (const hsrans_member_range *)cp.rows, cp.header + kPlanesWsRows, shape.set_rows, d_work, W * stride,
                                                              control + ws.set, workspace_bytes - ws.set, hip_stream);
    if (rc != HSRANS_OK)
      return rc;
  }

  // ---- the merge behind it ----
  uint32_t work_mask = 0;
  const PlanePtrs src = merge_sources(desc, pg->d_frame, d_work, stride, &work_mask);
  const hipError_t merged =
      base.on ? launch_planes_merge_indirect_delta(W, src, work_mask, cp.ranges, cp.header, cp.first_task, cp.base, base.d,
                                                   planes_merge_indirect_delta_grid(ctx->geom.num_cus, W, max_count, stride), d_out, s)
              : launch_planes_merge_indirect(W, src, work_mask, cp.ranges, cp.header, cp.first_task, cp.base, shape.merge_grid, d_out, s);
  if (merged != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_decode_device_planes_gather_indirect(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges, const uint32_t *d_count, uint32_t max_count,
                                                           uint64_t max_elements, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace,
                                                           size_t workspace_bytes, void *hip_stream)
{
  return planes_gather_indirect_flow(ctx, pg, d_ranges, d_count, max_count, max_elements, PlanesBase{}, d_out, out_capacity, d_work, work_bytes, d_workspace, workspace_bytes,
                                     hip_stream);
}

extern "C" int hsrans_decode_device_planes_gather_indirect_delta(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges, const uint32_t *d_count,
                                                                 uint32_t max_count, uint64_t max_elements, const void *d_base, size_t base_bytes, void *d_out,
                                                                 size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
  return planes_gather_indirect_flow(ctx, pg, d_ranges, d_count, max_count, max_elements, PlanesBase{true, d_base, base_bytes}, d_out, out_capacity, d_work, work_bytes,
                                     d_workspace, workspace_bytes, hip_stream);
}

extern "C" int hsrans_planes_gather_refused(hsrans_ctx *ctx, hsrans_planes_gather *pg, void *hip_stream)
try
{
  if (ctx == nullptr || pg == nullptr || pg->ctx != ctx)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  const int rc = refusal_word_take(pg->d_refused, (hipStream_t)hip_stream);
  if (rc != HSRANS_OK)
    return rc;
  // (the set's own word: the planes cut has passed every row the set sees, so this should never fire; it is reported if it does)
  return pg->set != nullptr ? hsrans_gather_set_refused(ctx, pg->set, hip_stream) : HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}
