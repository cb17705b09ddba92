// hsrans_capi_planes_pack.cpp — hsrans_pack_device and hsrans_planes_pack_device (include/hsrans_hip.h): many streams, or many frames of
// byte planes, into one exact-size arena in one call.  The layouts and the task prefix are pure host functions; the two entries check
// everything, build ONE table of PackItem records — a stream each, or every plane of every member in member and plane order — and queue
// ONE k_pack launch behind its upload (hsrans_planes_pack.hip).  The table goes through the context's task buffers as the planes batch's
// member tables do (launch_with_table, hsrans_capi_planes_batch.cpp: the gathers' protocol, gather_region_upload).
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"
#include "planes_cut_batch.h"

#include "hsrans_internal.h"

static_assert(sizeof(PackItem) == 32, "pack table layout");

namespace
{
constexpr uint32_t kMaxPackMembers = 65536;                           // the planes sets' members
constexpr uint32_t kMaxPackItems = kMaxPackMembers * HSRANS_PLANES_MAX; // ... and all their planes

// hsrans_planes_create's rules for a descriptor without the plans: the element size, offsets that are multiples of 16, lengths that are
// not 0, up16 spans that are disjoint, a frame_length not below the last byte.  *packed: the sum of the planes' up16(length).
bool pack_desc_ok(const hsrans_planes_desc &desc, uint64_t *packed)
{
  if (!planes_width_ok(desc.elem_size))
    return false;
  std::vector<Span> spans;
  uint64_t end = 0, sum = 0;
  for (uint32_t p = 0; p < desc.elem_size; p++)
  {
    const uint64_t offset = desc.offset[p], length = desc.length[p];
    if ((offset & 15) != 0 || length == 0 || length > ~(uint64_t)0 - 15 || offset + up16(length) < offset || sum + up16(length) < sum)
      return false;
    spans.push_back(Span{(uintptr_t)offset, (uintptr_t)(offset + up16(length)), true}); // (as writes: no two planes share bytes)
    end = std::max<uint64_t>(end, offset + length);
    sum += up16(length);
  }
  *packed = sum;
  return spans_disjoint(spans) && desc.frame_length >= end;
}

// What both entries do once their own arguments are checked: layer 1's rules over `count` sources, the overlap rule of the arena against
// the sources and against `also_read` (the frames the sources lie in), the table, and the one launch behind its upload under ctx->lock.
int pack_launch(hsrans_ctx *ctx, const void *const *d_srcs, const size_t *lengths, uint32_t count, void *d_arena, size_t arena_capacity,
                const std::vector<Span> &also_read, hipStream_t s)
{
  if (ctx == nullptr || d_srcs == nullptr || lengths == nullptr || count == 0 || count > kMaxPackItems)
    return HSRANS_E_ARG;
  std::vector<uint64_t> offsets((size_t)count + 1);
  std::vector<uint32_t> first_task((size_t)count + 1);
  const size_t total = hsrans_pack_layout(lengths, count, offsets.data());
  const size_t n_tasks = hsrans_pack_tasks(lengths, count, first_task.data());
  if (total == 0 || n_tasks == 0 || !aligned16(d_arena) || wraps(d_arena, arena_capacity) || arena_capacity < total)
    return HSRANS_E_ARG;
  std::vector<Span> spans(also_read);
  spans.reserve(spans.size() + count + 1);
  spans.push_back(span_of(d_arena, arena_capacity, true));
  for (uint32_t k = 0; k < count; k++)
  {
    if (!aligned16(d_srcs[k]) || wraps(d_srcs[k], lengths[k]))
      return HSRANS_E_ARG;
    spans.push_back(span_of(d_srcs[k], lengths[k], false));
  }
  if (!spans_disjoint(spans))
    return HSRANS_E_ARG;

  // the table is written where it is uploaded from: no copy of it on the host
  std::lock_guard<std::mutex> lk(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  return gather_region_upload(
      ctx, (size_t)count * sizeof(PackItem), s,
      [&](uint8_t *host) {
        PackItem *table = (PackItem *)host;
        for (uint32_t k = 0; k < count; k++)
          table[k] = PackItem{(const uint8_t *)d_srcs[k], (uint8_t *)d_arena + offsets[k], lengths[k], first_task[k], 0};
        return HSRANS_OK;
      },
      [&](const uint8_t *dev) { return launch_pack((const PackItem *)dev, count, (uint32_t)n_tasks, s); });
}
} // namespace

extern "C" size_t hsrans_pack_layout(const size_t *lengths, uint32_t count, uint64_t *offsets)
{
  if (lengths == nullptr || count == 0 || count > kMaxPackItems)
    return 0;
  size_t total = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    if (lengths[k] == 0 || lengths[k] > ~(size_t)0 - 15 || total + up16(lengths[k]) < total)
      return 0;
    total += up16(lengths[k]);
  }
  if (offsets != nullptr)
  {
    uint64_t at = 0;
    for (uint32_t k = 0; k < count; k++)
    {
      offsets[k] = at;
      at += up16(lengths[k]);
    }
    offsets[count] = at;
  }
  return total;
}

extern "C" size_t hsrans_pack_tasks(const size_t *lengths, uint32_t count, uint32_t *first_task)
{
  if (hsrans_pack_layout(lengths, count, nullptr) == 0)
    return 0;
  uint64_t total = 0; // (the up16 lengths sum to less than 2^64: their chunks to less than 2^52 + count)
  for (uint32_t k = 0; k < count; k++)
    total += pack_tasks_of(lengths[k]);
  if (total >= 0x80000000u)
    return 0;
  if (first_task != nullptr)
  {
    uint32_t at = 0;
    for (uint32_t k = 0; k < count; k++)
    {
      first_task[k] = at;
      at += (uint32_t)pack_tasks_of(lengths[k]);
    }
    first_task[count] = at;
  }
  return (size_t)total;
}

extern "C" int hsrans_pack_device(hsrans_ctx *ctx, const void *const *d_srcs, const size_t *lengths, uint32_t count, void *d_arena, size_t arena_capacity,
                                  void *hip_stream)
try
{
  return pack_launch(ctx, d_srcs, lengths, count, d_arena, arena_capacity, {}, (hipStream_t)hip_stream);
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

extern "C" size_t hsrans_planes_pack_layout(const hsrans_planes_desc *descs, uint32_t count, hsrans_planes_desc *out_descs, uint64_t *bases)
try
{
  if (descs == nullptr || count == 0 || count > kMaxPackMembers)
    return 0;
  std::vector<uint64_t> packed(count);
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    if (!pack_desc_ok(descs[k], &packed[k]) || total + packed[k] < total)
      return 0;
    total += packed[k];
  }
  if (total > ~(size_t)0)
    return 0;
  uint64_t base = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    if (out_descs != nullptr)
    {
      hsrans_planes_desc d = descs[k]; // (read whole before it is written: out_descs may be descs)
      uint64_t at = 0;
      for (uint32_t p = 0; p < d.elem_size; p++)
      {
        d.offset[p] = at;
        d.frame_length = at + d.length[p];
        at += up16(d.length[p]);
      }
      out_descs[k] = d;
    }
    if (bases != nullptr)
      bases[k] = base;
    base += packed[k];
  }
  if (bases != nullptr)
    bases[count] = base;
  return (size_t)total;
}
catch (...)
{
  return 0;
}

extern "C" int hsrans_planes_pack_device(hsrans_ctx *ctx, const hsrans_planes_desc *descs, const void *const *d_frames, const size_t *frame_lengths, uint32_t count,
                                         void *d_arena, size_t arena_capacity, void *hip_stream, hsrans_planes_desc *out_descs, uint64_t *bases)
try
{
  const auto failed = [&](int rc) { // every output of a call that did not pack: no descriptor
    if (out_descs != nullptr && count != 0)
      memset(out_descs, 0, (size_t)count * sizeof(hsrans_planes_desc));
    return rc;
  };
  if (ctx == nullptr || descs == nullptr || d_frames == nullptr || frame_lengths == nullptr || out_descs == nullptr || d_arena == nullptr)
    return failed(HSRANS_E_ARG);
  if (hsrans_planes_pack_layout(descs, count, nullptr, nullptr) == 0)
    return failed(HSRANS_E_ARG);

  // ---- layer 1's items: every plane of every member, in member and plane order ----
  std::vector<const void *> srcs;
  std::vector<size_t> lengths;
  std::vector<Span> frames;
  srcs.reserve((size_t)count * 2);
  lengths.reserve((size_t)count * 2);
  frames.reserve(count);
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_planes_desc &desc = descs[k];
    if (!aligned16(d_frames[k]) || frame_lengths[k] < desc.frame_length || wraps(d_frames[k], frame_lengths[k]))
      return failed(HSRANS_E_ARG);
    frames.push_back(span_of(d_frames[k], frame_lengths[k], false));
    for (uint32_t p = 0; p < desc.elem_size; p++)
    {
      srcs.push_back((const uint8_t *)d_frames[k] + desc.offset[p]);
      lengths.push_back((size_t)desc.length[p]);
    }
  }
  // (the launch first: out_descs may be descs, and a refusal must not leave half of the layout behind)
  const int rc = pack_launch(ctx, srcs.data(), lengths.data(), (uint32_t)srcs.size(), d_arena, arena_capacity, frames, (hipStream_t)hip_stream);
  if (rc != HSRANS_OK)
    return failed(rc);
  hsrans_planes_pack_layout(descs, count, out_descs, bases);
  return HSRANS_OK;
}
catch (...)
{
  if (out_descs != nullptr && count != 0)
    memset(out_descs, 0, (size_t)count * sizeof(hsrans_planes_desc));
  return HSRANS_E_HIP;
}
