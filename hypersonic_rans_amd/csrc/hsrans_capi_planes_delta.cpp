// hsrans_capi_planes_delta.cpp — hsrans_*_device_planes_delta (include/hsrans_hip.h): tensors coded against a base.  A delta frame of `in`
// against `base` is byte for byte the ordinary frame of in ^ base, so nothing of the frame, the descriptor or the codec is new: the XOR rides
// in the split and the merge kernels (hsrans_planes_delta.hip), and every entry here is its plain counterpart's own body — planes_*_flow,
// hsrans_internal.h — run with a base.  What this file adds is the rule on the host in plain C++ (hsrans_planes_split_delta / _merge_delta),
// the two kernels alone, and the entries' hand-over of the base to the flows.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"
#include "planes_cut_batch.h"

#include "hsrans_internal.h"

namespace
{
bool host_args_ok(uint32_t elem_size, const void *elements, const void *base, const uint8_t *const *planes)
{
  if (!planes_width_ok(elem_size) || elements == nullptr || base == nullptr || planes == nullptr)
    return false;
  for (uint32_t p = 0; p < elem_size; p++)
    if (planes[p] == nullptr)
      return false;
  return true;
}

// the checks of the two kernel entries: hsrans_planes_split_device's, with the base a read span of the element buffer's size.  The merge's
// element buffer is written and may be the base itself; the split's is read, and reads may share.
bool kernel_args_ok(uint32_t W, const void *d_elements, const void *d_base, size_t elements, const void *const *d_planes, bool planes_written, PlanePtrs *pp)
{
  if (!planes_width_ok(W) || !aligned16(d_elements) || d_planes == nullptr || elements == 0 || elements > kPlanesMaxElements)
    return false;
  std::vector<Span> spans;
  spans.push_back(span_of(d_elements, elements * W, !planes_written));
  if (!planes_base_spans(PlanesBase{true, d_base, elements * W}, W, elements, planes_written ? nullptr : d_elements, elements * W, &spans))
    return false;
  for (uint32_t p = 0; p < W; p++)
  {
    if (!aligned16(d_planes[p]))
      return false;
    pp->p[p] = (uint8_t *)d_planes[p];
    spans.push_back(span_of(d_planes[p], elements, true)); // (as writes on either side: two planes never share memory)
  }
  return spans_disjoint(spans);
}
} // namespace

extern "C" int hsrans_planes_split_delta(uint32_t elem_size, const void *in, const void *base, size_t elements, uint8_t *const *planes)
{
  if (!host_args_ok(elem_size, in, base, planes))
    return HSRANS_E_ARG;
  const uint8_t *src = (const uint8_t *)in, *b = (const uint8_t *)base;
  for (size_t i = 0; i < elements; i++)
    for (uint32_t p = 0; p < elem_size; p++)
      planes[p][i] = src[i * elem_size + p] ^ b[i * elem_size + p];
  return HSRANS_OK;
}

extern "C" int hsrans_planes_merge_delta(uint32_t elem_size, const uint8_t *const *planes, const void *base, size_t elements, void *out)
{
  if (!host_args_ok(elem_size, out, base, planes))
    return HSRANS_E_ARG;
  const uint8_t *b = (const uint8_t *)base; // (may be `out`: every byte is read, then written)
  uint8_t *dst = (uint8_t *)out;
  for (size_t i = 0; i < elements; i++)
    for (uint32_t p = 0; p < elem_size; p++)
      dst[i * elem_size + p] = planes[p][i] ^ b[i * elem_size + p];
  return HSRANS_OK;
}

extern "C" int hsrans_planes_split_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const void *d_base, size_t elements, void *const *d_planes,
                                                void *hip_stream)
try
{
  PlanePtrs pp{};
  if (ctx == nullptr || !kernel_args_ok(elem_size, d_in, d_base, elements, (const void *const *)d_planes, true, &pp))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_split_delta(elem_size, d_in, d_base, elements, pp, (hipStream_t)hip_stream) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_merge_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const void *d_base, size_t elements, void *d_out,
                                                void *hip_stream)
try
{
  PlanePtrs pp{};
  if (ctx == nullptr || !kernel_args_ok(elem_size, d_out, d_base, elements, d_planes, false, &pp))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_merge_delta(elem_size, pp, d_base, elements, d_out, (hipStream_t)hip_stream) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" size_t hsrans_encode_device_planes_delta(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const void *d_base, size_t base_bytes,
                                                    size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags,
                                                    void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc, hsrans_dplan **out_dplans)
{
  return planes_encode_flow(ctx, elem_size, states, bits, d_in, PlanesBase{true, d_base, base_bytes}, elements, d_frame, frame_capacity, block_size, index_interval, flags,
                            d_work, work_bytes, hip_stream, desc, out_dplans);
}

extern "C" int hsrans_decode_device_planes_delta(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const void *d_base, size_t base_bytes,
                                                 void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_decode_flow(ctx, planes, d_frame, frame_length, PlanesBase{true, d_base, base_bytes}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_encode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases, const size_t *base_bytes, uint32_t count,
                                                       void *d_work, size_t work_bytes, void *hip_stream, hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats)
{
  return planes_encode_batch_flow(ctx, members, d_bases, base_bytes, true, count, d_work, work_bytes, hip_stream, out_dplans, stats);
}

extern "C" int hsrans_decode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                                       const void *const *d_bases, const size_t *base_bytes, void *const *d_outs, const size_t *out_capacities, void *d_work,
                                                       size_t work_bytes, void *hip_stream)
{
  return planes_decode_batch_flow(ctx, set, d_frames, frame_lengths, d_bases, base_bytes, true, d_outs, out_capacities, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_gather_delta(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const void *d_base,
                                                        size_t base_bytes, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_gather_flow(ctx, pg, ranges, count, PlanesBase{true, d_base, base_bytes}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}
