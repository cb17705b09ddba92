// hsrans_capi_planes.cpp — multi-byte elements coded as byte planes: the element layer over the batch entries.  Part of the C ABI of
// libhsrans_hip.so (include/hsrans_hip.h).  hsrans_encode_device_planes is one split launch (hsrans_planes.hip), ONE hsrans_encode_device_batch
// of the planes as mt_ members and, where asked for, a copy over the planes that did not shrink; hsrans_decode_device_planes is
// hsrans_decode_device_batch of the coded planes and one merge launch behind it.  Both codecs are used as they are, through their public
// entries: a coded plane is byte for byte what hsrans_encode_device(HSRANS_MT, ...) writes for the plane's bytes.
// The two entries' bodies are planes_encode_flow and planes_decode_flow (hsrans_internal.h), which take an optional base: without one they are
// the entries as they always were; with one the split or the merge is the delta kernel (hsrans_planes_base.hip).
// hsrans_*_device_planes_delta — tensors coded against a base — are these entries given a base, each beside its plain form (here, and in
// hsrans_capi_planes_batch.cpp and hsrans_capi_planes_gather.cpp).  A delta frame of `in` against `base` is byte for byte the ordinary frame
// of in ^ base, so nothing of the frame, the descriptor or the codec is new: the XOR rides in the split and the merge.
// hsrans_*_device_planes_diff are the delta entries under the other residue rule (PlanesBase::rule): the zigzag of the elements' wrapped
// difference in place of the XOR, by the _diff kernels of the same unit; every check, span and launch count is the delta path's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"
#include "planes_cut_batch.h"

#include "hsrans_internal.h"

namespace
{
constexpr uint32_t kMaxBatchTasks = 1u << 24; // hsrans_encode_device_batch: fewer mt_ blocks than this in one call

size_t plane_stride(int states, size_t elements) { return up256(capacity(HSRANS_MT, states, elements)); } // a coded plane's room in the frame

// the planes of a workspace: plane p at p * up256(elements)
PlanePtrs work_planes(uint32_t W, void *d_work, size_t elements)
{
  PlanePtrs pp{};
  for (uint32_t p = 0; p < W; p++)
    pp.p[p] = (uint8_t *)d_work + p * up256(elements);
  return pp;
}

// the checks of the kernel entries: W pointers to `elements` bytes each and the element buffer, all 16-byte aligned, none meeting another.
// base.on: the base joins them as a read span of the element buffer's size.  The merge's element buffer is written and may be the base
// itself; the split's is read, and reads may share.
bool kernel_args_ok(uint32_t W, const void *d_elements, const PlanesBase &base, size_t elements, const void *const *d_planes, bool planes_written, PlanePtrs *pp)
{
  if (!planes_width_ok(W) || !aligned16(d_elements) || d_planes == nullptr || elements == 0 || elements > kPlanesMaxElements)
    return false;
  std::vector<Span> spans;
  spans.push_back(span_of(d_elements, elements * W, !planes_written));
  if (!planes_base_spans(base, W, elements, planes_written ? nullptr : d_elements, elements * W, &spans))
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

void drop_plans(hsrans_dplan **plans, uint32_t W)
{
  for (uint32_t p = 0; plans != nullptr && p < W; p++)
    if (plans[p] != nullptr)
    {
      hsrans_dplan_destroy(plans[p]);
      plans[p] = nullptr;
    }
}
} // namespace

bool planes_encode_check(uint32_t W, int states, uint32_t bits, const void *d_in, size_t elements, const void *d_frame, size_t frame_capacity, uint32_t block_size,
                         uint32_t index_interval, uint32_t flags, bool want_plans, PlanesEncShape *out)
{
  if (!planes_width_ok(W) || (flags & ~HSRANS_PLANES_STORE_INCOMPRESSIBLE) != 0 || !aligned16(d_in) || !aligned16(d_frame))
    return false;
  if (!(states == 32 || states == 64) || elements == 0 || elements > kPlanesMaxElements)
    return false;
  out->stride = plane_stride(states, elements);
  out->work_stride = up256(elements);
  EncShape sh;
  if (!mt_shape(states, bits, elements, out->stride, block_size, index_interval, want_plans, &sh) || frame_capacity < W * out->stride)
    return false;
  out->n_blocks = sh.n_blocks;
  return true;
}

int planes_desc_check(const hsrans_ctx *ctx, const hsrans_planes_desc *desc, hsrans_dplan *const *dplans)
{
  if (ctx == nullptr || desc == nullptr || dplans == nullptr || !planes_width_ok(desc->elem_size) || !valid_codec(HSRANS_MT, (int)desc->states, desc->bits) ||
      desc->elements == 0 || desc->elements > kPlanesMaxElements || (desc->stored_mask >> desc->elem_size) != 0)
    return HSRANS_E_ARG;
  const uint32_t W = desc->elem_size;
  std::vector<Span> spans;
  uint64_t end = 0;
  for (uint32_t p = 0; p < W; p++)
  {
    const bool is_stored = (desc->stored_mask >> p) & 1;
    const hsrans_dplan *d = dplans[p];
    if ((desc->offset[p] & 15) != 0 || desc->length[p] == 0 || desc->offset[p] + desc->length[p] < desc->offset[p] || is_stored != (d == nullptr))
      return HSRANS_E_ARG;
    if (is_stored ? desc->length[p] != desc->elements
                  : (d->ctx != ctx || d->hdr.decoded_len != desc->elements || d->hdr.stream_len != desc->length[p] || d->hdr.states != desc->states ||
                     d->hdr.bits != desc->bits))
      return HSRANS_E_ARG;
    spans.push_back(Span{(uintptr_t)desc->offset[p], (uintptr_t)(desc->offset[p] + up16(desc->length[p])), true}); // (as writes: no two planes share bytes)
    end = std::max<uint64_t>(end, desc->offset[p] + desc->length[p]);
  }
  if (!spans_disjoint(spans) || desc->frame_length < end)
    return HSRANS_E_ARG;
  return HSRANS_OK;
}

extern "C" size_t hsrans_planes_capacity(uint32_t elem_size, int states, size_t elements)
{
  if (!planes_width_ok(elem_size) || (states != 32 && states != 64) || elements == 0)
    return 0;
  return elem_size * plane_stride(states, elements);
}

extern "C" size_t hsrans_planes_workspace_bytes(uint32_t elem_size, size_t elements)
{
  if (!planes_width_ok(elem_size) || elements == 0)
    return 0;
  return elem_size * up256(elements);
}

// ---- the split and the merge alone, on the host in plain C++ and as one kernel: each plain entry is the delta entry's body without a base ----
namespace
{
bool host_args_ok(uint32_t elem_size, const void *elements, const uint8_t *const *planes)
{
  if (!planes_width_ok(elem_size) || elements == nullptr || planes == nullptr)
    return false;
  for (uint32_t p = 0; p < elem_size; p++)
    if (planes[p] == nullptr)
      return false;
  return true;
}

// element i of a tensor of W-byte elements as the little-endian unsigned integer the diff rule reads it as
uint64_t host_element(const uint8_t *elements, size_t i, uint32_t W)
{
  uint64_t v = 0;
  for (uint32_t p = 0; p < W; p++)
    v |= (uint64_t)elements[i * W + p] << (8 * p);
  return v;
}

// base: null, or what is XORed into every byte on its way (PlanesRule::kXor), or what is subtracted from every element, modulo 2^(8 W),
// before the difference's sign is folded into its lowest bit (PlanesRule::kDiff)
int host_split(uint32_t elem_size, const void *in, const void *base, PlanesRule rule, size_t elements, uint8_t *const *planes)
{
  if (!host_args_ok(elem_size, in, planes))
    return HSRANS_E_ARG;
  const uint8_t *src = (const uint8_t *)in, *b = (const uint8_t *)base;
  if (b != nullptr && rule == PlanesRule::kDiff)
  {
    const uint32_t top = 8 * elem_size - 1; // (a bit above 8 W - 1 of z is never stored: only its low W bytes are)
    for (size_t i = 0; i < elements; i++)
    {
      const uint64_t d = host_element(src, i, elem_size) - host_element(b, i, elem_size);
      const uint64_t z = (d << 1) ^ (0 - ((d >> top) & 1));
      for (uint32_t p = 0; p < elem_size; p++)
        planes[p][i] = (uint8_t)(z >> (8 * p));
    }
    return HSRANS_OK;
  }
  for (size_t i = 0; i < elements; i++)
    for (uint32_t p = 0; p < elem_size; p++)
      planes[p][i] = src[i * elem_size + p] ^ (b != nullptr ? b[i * elem_size + p] : 0);
  return HSRANS_OK;
}

int host_merge(uint32_t elem_size, const uint8_t *const *planes, const void *base, PlanesRule rule, size_t elements, void *out)
{
  if (!host_args_ok(elem_size, out, planes))
    return HSRANS_E_ARG;
  const uint8_t *b = (const uint8_t *)base; // (may be `out`: every byte, or with kDiff every element, is read, then written)
  uint8_t *dst = (uint8_t *)out;
  if (b != nullptr && rule == PlanesRule::kDiff)
  {
    const uint64_t low = elem_size == 8 ? ~(uint64_t)0 : ((uint64_t)1 << (8 * elem_size)) - 1;
    for (size_t i = 0; i < elements; i++)
    {
      uint64_t z = 0;
      for (uint32_t p = 0; p < elem_size; p++)
        z |= (uint64_t)planes[p][i] << (8 * p);
      const uint64_t d = ((z >> 1) ^ (0 - (z & 1))) & low, v = host_element(b, i, elem_size) + d;
      for (uint32_t p = 0; p < elem_size; p++)
        dst[i * elem_size + p] = (uint8_t)(v >> (8 * p));
    }
    return HSRANS_OK;
  }
  for (size_t i = 0; i < elements; i++)
    for (uint32_t p = 0; p < elem_size; p++)
      dst[i * elem_size + p] = planes[p][i] ^ (b != nullptr ? b[i * elem_size + p] : 0);
  return HSRANS_OK;
}

int split_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const PlanesBase &base, size_t elements, void *const *d_planes, void *hip_stream)
try
{
  PlanePtrs pp{};
  if (ctx == nullptr || !kernel_args_ok(elem_size, d_in, base, elements, (const void *const *)d_planes, true, &pp))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_split(elem_size, d_in, base.on ? base.d : nullptr, base.rule, elements, pp, (hipStream_t)hip_stream) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

int merge_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const PlanesBase &base, size_t elements, void *d_out, void *hip_stream)
try
{
  PlanePtrs pp{};
  if (ctx == nullptr || !kernel_args_ok(elem_size, d_out, base, elements, d_planes, false, &pp))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_merge(elem_size, pp, base.on ? base.d : nullptr, base.rule, elements, d_out, (hipStream_t)hip_stream) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}
} // namespace

extern "C" int hsrans_planes_split(uint32_t elem_size, const void *in, size_t elements, uint8_t *const *planes)
{
  return host_split(elem_size, in, nullptr, PlanesRule::kXor, elements, planes);
}

extern "C" int hsrans_planes_split_delta(uint32_t elem_size, const void *in, const void *base, size_t elements, uint8_t *const *planes)
{
  return base == nullptr ? HSRANS_E_ARG : host_split(elem_size, in, base, PlanesRule::kXor, elements, planes);
}

extern "C" int hsrans_planes_merge(uint32_t elem_size, const uint8_t *const *planes, size_t elements, void *out)
{
  return host_merge(elem_size, planes, nullptr, PlanesRule::kXor, elements, out);
}

extern "C" int hsrans_planes_merge_delta(uint32_t elem_size, const uint8_t *const *planes, const void *base, size_t elements, void *out)
{
  return base == nullptr ? HSRANS_E_ARG : host_merge(elem_size, planes, base, PlanesRule::kXor, elements, out);
}

extern "C" int hsrans_planes_split_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, size_t elements, void *const *d_planes, void *hip_stream)
{
  return split_device(ctx, elem_size, d_in, PlanesBase{}, elements, d_planes, hip_stream);
}

// (a null d_base is refused with the base's other checks, planes_base_spans; elements * elem_size: read only once both are known to be in range)
extern "C" int hsrans_planes_split_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const void *d_base, size_t elements, void *const *d_planes,
                                                void *hip_stream)
{
  return split_device(ctx, elem_size, d_in, PlanesBase{true, d_base, elements * elem_size}, elements, d_planes, hip_stream);
}

extern "C" int hsrans_planes_merge_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, size_t elements, void *d_out, void *hip_stream)
{
  return merge_device(ctx, elem_size, d_planes, PlanesBase{}, elements, d_out, hip_stream);
}

extern "C" int hsrans_planes_merge_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const void *d_base, size_t elements, void *d_out,
                                                void *hip_stream)
{
  return merge_device(ctx, elem_size, d_planes, PlanesBase{true, d_base, elements * elem_size}, elements, d_out, hip_stream);
}

// ---- the diff forms of the four entries above: the delta entries' bodies under the other residue rule ----
extern "C" int hsrans_planes_split_diff(uint32_t elem_size, const void *in, const void *base, size_t elements, uint8_t *const *planes)
{
  return base == nullptr ? HSRANS_E_ARG : host_split(elem_size, in, base, PlanesRule::kDiff, elements, planes);
}

extern "C" int hsrans_planes_merge_diff(uint32_t elem_size, const uint8_t *const *planes, const void *base, size_t elements, void *out)
{
  return base == nullptr ? HSRANS_E_ARG : host_merge(elem_size, planes, base, PlanesRule::kDiff, elements, out);
}

extern "C" int hsrans_planes_split_diff_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const void *d_base, size_t elements, void *const *d_planes,
                                               void *hip_stream)
{
  return split_device(ctx, elem_size, d_in, PlanesBase{true, d_base, elements * elem_size, PlanesRule::kDiff}, elements, d_planes, hip_stream);
}

extern "C" int hsrans_planes_merge_diff_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const void *d_base, size_t elements, void *d_out,
                                               void *hip_stream)
{
  return merge_device(ctx, elem_size, d_planes, PlanesBase{true, d_base, elements * elem_size, PlanesRule::kDiff}, elements, d_out, hip_stream);
}

bool planes_base_spans(const PlanesBase &base, uint32_t W, size_t elements, const void *d_out, size_t out_capacity, std::vector<Span> *spans)
{
  if (!base.on)
    return true;
  if (!aligned16(base.d) || base.bytes < elements * W || wraps(base.d, base.bytes))
    return false;
  if (d_out != nullptr && base.d == d_out && out_capacity <= base.bytes) // in place: the output's span stands for the base's bytes it covers
    spans->push_back(span_of((const uint8_t *)base.d + out_capacity, base.bytes - out_capacity, false));
  else
    spans->push_back(span_of(base.d, base.bytes, false));
  return true;
}

bool planes_base_meets_frame(const PlanesBase &base, const void *d_frame, size_t frame_length)
{
  if (!base.on)
    return false;
  std::vector<Span> frames{span_of(d_frame, frame_length, false)};
  return spans_meet({span_of(base.d, base.bytes, false)}, frames);
}

size_t planes_encode_flow(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const PlanesBase &base, size_t elements, void *d_frame,
                          size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags, void *d_work, size_t work_bytes, void *hip_stream,
                          hsrans_planes_desc *desc, hsrans_dplan **out_dplans)
try
{
  if (desc != nullptr)
    *desc = hsrans_planes_desc{};
  if (!planes_width_ok(elem_size))
    return 0;
  const uint32_t W = elem_size;
  for (uint32_t p = 0; out_dplans != nullptr && p < W; p++)
    out_dplans[p] = nullptr; // (the caller's array may hold anything: nothing to destroy yet)
  if (ctx == nullptr || desc == nullptr || !aligned16(d_work))
    return 0;

  // ---- everything checked before anything is launched: each plane by its single call's rules (mt_shape), then the call's own ----
  PlanesEncShape ps;
  if (!planes_encode_check(W, states, bits, d_in, elements, d_frame, frame_capacity, block_size, index_interval, flags, out_dplans != nullptr, &ps) ||
      (uint64_t)ps.n_blocks * W >= kMaxBatchTasks)
    return 0;
  const size_t stride = ps.stride, work_stride = ps.work_stride;
  Carve frame, work; // (the frame and the workspace: W regions each)
  size_t offset[HSRANS_PLANES_MAX] = {};
  for (uint32_t p = 0; p < W; p++)
  {
    offset[p] = frame.take(stride, 256);
    work.take(work_stride, 256);
  }
  if (frame_capacity < frame.close(256) || work_bytes < work.close(256))
    return 0;
  {
    std::vector<Span> spans{span_of(d_in, elements * W, false), span_of(d_frame, frame_capacity, true), span_of(d_work, work_bytes, true)};
    if (!planes_base_spans(base, W, elements, nullptr, 0, &spans) || !spans_disjoint(spans))
      return 0;
  }

  hipStream_t s = (hipStream_t)hip_stream;
  const PlanePtrs pp = work_planes(W, d_work, elements);
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_split(W, d_in, base.on ? base.d : nullptr, base.rule, elements, pp, s) != hipSuccess)
  {
    (void)hipGetLastError();
    return 0;
  }
  // (ctx->lock is not held here: hsrans_encode_device_batch takes it, and it is not recursive)
  hsrans_encode_member members[HSRANS_PLANES_MAX] = {};
  for (uint32_t p = 0; p < W; p++)
  {
    hsrans_encode_member &m = members[p];
    m.container = HSRANS_MT;
    m.states = states;
    m.bits = bits;
    m.block_size = block_size;
    m.d_in = pp.p[p];
    m.length = elements;
    m.d_out = (uint8_t *)d_frame + offset[p];
    m.out_capacity = stride;
    m.index_interval = index_interval;
  }
  if (hsrans_encode_device_batch(ctx, members, W, hip_stream, out_dplans, nullptr) != HSRANS_OK)
  {
    drop_plans(out_dplans, W);
    return 0;
  }

  // ---- the planes that did not shrink: their bytes instead of their streams ----
  uint32_t stored = 0;
  bool copied = true;
  for (uint32_t p = 0; p < W; p++)
    if ((flags & HSRANS_PLANES_STORE_INCOMPRESSIBLE) != 0 && members[p].stream_length >= elements)
    {
      stored |= 1u << p;
      copied = copied && hipMemcpyAsync(members[p].d_out, pp.p[p], elements, hipMemcpyDeviceToDevice, s) == hipSuccess;
    }
  if (stored != 0 && !stream_settle(s, copied))
  {
    drop_plans(out_dplans, W);
    return 0;
  }

  desc->elem_size = W;
  desc->states = (uint32_t)states;
  desc->bits = bits;
  desc->block_size = block_size;
  desc->index_interval = index_interval;
  desc->stored_mask = stored;
  desc->elements = elements;
  for (uint32_t p = 0; p < W; p++)
  {
    const bool is_stored = (stored >> p) & 1;
    desc->offset[p] = offset[p];
    desc->length[p] = is_stored ? elements : members[p].stream_length;
    desc->frame_length = offset[p] + desc->length[p];
    if (is_stored && out_dplans != nullptr && out_dplans[p] != nullptr)
    {
      hsrans_dplan_destroy(out_dplans[p]);
      out_dplans[p] = nullptr;
    }
  }
  return (size_t)desc->frame_length;
}
catch (...) // (thrown only after the caller's arrays were reset, or before elem_size was seen to be valid: then they were not touched)
{
  if (desc != nullptr)
    *desc = hsrans_planes_desc{};
  if (planes_width_ok(elem_size))
    drop_plans(out_dplans, elem_size);
  return 0;
}

extern "C" size_t hsrans_encode_device_planes(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, size_t elements, void *d_frame,
                                              size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags, void *d_work, size_t work_bytes,
                                              void *hip_stream, hsrans_planes_desc *desc, hsrans_dplan **out_dplans)
{
  return planes_encode_flow(ctx, elem_size, states, bits, d_in, PlanesBase{}, elements, d_frame, frame_capacity, block_size, index_interval, flags, d_work, work_bytes,
                            hip_stream, desc, out_dplans);
}

extern "C" size_t hsrans_encode_device_planes_delta(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const void *d_base, size_t base_bytes,
                                                    size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags,
                                                    void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc, hsrans_dplan **out_dplans)
{
  return planes_encode_flow(ctx, elem_size, states, bits, d_in, PlanesBase{true, d_base, base_bytes}, elements, d_frame, frame_capacity, block_size, index_interval, flags,
                            d_work, work_bytes, hip_stream, desc, out_dplans);
}

extern "C" size_t hsrans_encode_device_planes_diff(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const void *d_base, size_t base_bytes,
                                                   size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags,
                                                   void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc, hsrans_dplan **out_dplans)
{
  return planes_encode_flow(ctx, elem_size, states, bits, d_in, PlanesBase{true, d_base, base_bytes, PlanesRule::kDiff}, elements, d_frame, frame_capacity, block_size,
                            index_interval, flags, d_work, work_bytes, hip_stream, desc, out_dplans);
}

extern "C" void hsrans_planes_destroy(hsrans_planes *planes)
{
  if (planes == nullptr)
    return;
  if (planes->batch != nullptr)
    hsrans_dplan_batch_destroy(planes->batch);
  delete planes;
}

extern "C" int hsrans_planes_create(hsrans_ctx *ctx, const hsrans_planes_desc *desc, hsrans_dplan *const *dplans, hsrans_planes **out_planes)
try
{
  if (out_planes == nullptr)
    return HSRANS_E_ARG;
  *out_planes = nullptr;
  if (planes_desc_check(ctx, desc, dplans) != HSRANS_OK)
    return HSRANS_E_ARG;
  const uint32_t W = desc->elem_size;

  hsrans_planes *pl = new (std::nothrow) hsrans_planes;
  if (pl == nullptr)
    return HSRANS_E_HIP;
  struct Guard // (an exception on its way to the handler below must not leak the object and its batch)
  {
    hsrans_planes *pl;
    bool armed = true;
    ~Guard()
    {
      if (armed)
        hsrans_planes_destroy(pl);
    }
  } guard{pl};
  pl->ctx = ctx;
  pl->desc = *desc;
  for (uint32_t p = 0; p < W; p++)
    if (dplans[p] != nullptr)
    {
      pl->coded.push_back(p);
      pl->dplans.push_back(dplans[p]);
    }
  if (!pl->coded.empty())
  {
    const int rc = hsrans_dplan_batch_create(ctx, pl->dplans.data(), (uint32_t)pl->dplans.size(), &pl->batch); // (refuses a plan that appears twice)
    if (rc != HSRANS_OK)
      return rc;
  }
  guard.armed = false;
  *out_planes = pl;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

int planes_decode_flow(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const PlanesBase &base, void *d_out, size_t out_capacity,
                       void *d_work, size_t work_bytes, void *hip_stream)
try
{
  if (ctx == nullptr || planes == nullptr || planes->ctx != ctx || !aligned16(d_frame) || !aligned16(d_out) || !aligned16(d_work))
    return HSRANS_E_ARG;
  const hsrans_planes_desc &desc = planes->desc;
  const uint32_t W = desc.elem_size;
  const size_t elements = (size_t)desc.elements;
  if (frame_length < desc.frame_length || out_capacity < elements * W || work_bytes < hsrans_planes_workspace_bytes(W, elements))
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans{span_of(d_frame, frame_length, false), span_of(d_out, out_capacity, true), span_of(d_work, work_bytes, true)};
    if (!planes_base_spans(base, W, elements, d_out, out_capacity, &spans) || !spans_disjoint(spans) || planes_base_meets_frame(base, d_frame, frame_length))
      return HSRANS_E_ARG;
  }
  // the merge's sources: a coded plane decoded into the workspace, a stored one where it lies in the frame
  PlanePtrs src = work_planes(W, d_work, elements);
  for (uint32_t p = 0; p < W; p++)
    if ((desc.stored_mask >> p) & 1)
      src.p[p] = (uint8_t *)d_frame + desc.offset[p];
  if (planes->batch != nullptr)
  {
    const void *streams[HSRANS_PLANES_MAX];
    void *outs[HSRANS_PLANES_MAX];
    size_t lengths[HSRANS_PLANES_MAX], caps[HSRANS_PLANES_MAX];
    for (size_t k = 0; k < planes->coded.size(); k++)
    {
      const uint32_t p = planes->coded[k];
      streams[k] = (const uint8_t *)d_frame + desc.offset[p];
      lengths[k] = (size_t)desc.length[p];
      outs[k] = src.p[p];
      caps[k] = elements;
    }
    const int rc = hsrans_decode_device_batch(ctx, planes->batch, streams, lengths, outs, caps, hip_stream);
    if (rc != HSRANS_OK)
      return rc;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (hipSetDevice(ctx->device) != hipSuccess || launch_planes_merge(W, src, base.on ? base.d : nullptr, base.rule, elements, d_out, s) != hipSuccess)
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

extern "C" int hsrans_decode_device_planes(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, void *d_out, size_t out_capacity,
                                           void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_decode_flow(ctx, planes, d_frame, frame_length, PlanesBase{}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_delta(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const void *d_base, size_t base_bytes,
                                                 void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_decode_flow(ctx, planes, d_frame, frame_length, PlanesBase{true, d_base, base_bytes}, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_diff(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const void *d_base, size_t base_bytes,
                                                void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_decode_flow(ctx, planes, d_frame, frame_length, PlanesBase{true, d_base, base_bytes, PlanesRule::kDiff}, d_out, out_capacity, d_work, work_bytes,
                            hip_stream);
}

extern "C" int hsrans_planes_status(hsrans_ctx *ctx, hsrans_planes *planes, void *hip_stream, int *plane_status)
try
{
  if (ctx == nullptr || planes == nullptr || planes->ctx != ctx)
    return HSRANS_E_ARG;
  for (uint32_t p = 0; plane_status != nullptr && p < planes->desc.elem_size; p++)
    plane_status[p] = HSRANS_OK;
  if (planes->batch == nullptr) // (every plane stored: nothing to report, but the call still waits for the stream as the batch's does)
    return hipSetDevice(ctx->device) == hipSuccess && stream_settle((hipStream_t)hip_stream, true) ? HSRANS_OK : HSRANS_E_HIP;
  int member_status[HSRANS_PLANES_MAX] = {};
  const int rc = hsrans_dplan_batch_status(ctx, planes->batch, hip_stream, member_status);
  for (size_t k = 0; plane_status != nullptr && k < planes->coded.size(); k++)
    plane_status[planes->coded[k]] = member_status[k];
  return rc;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_info(const hsrans_planes *planes, hsrans_planes_info_t *info)
try
{
  if (planes == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  *info = hsrans_planes_info_t{};
  info->coded = (uint32_t)planes->coded.size();
  info->stored = planes->desc.elem_size - info->coded;
  hsrans_batch_info bi{};
  if (planes->batch != nullptr && hsrans_dplan_batch_info(planes->batch, &bi) != HSRANS_OK)
    return HSRANS_E_HIP;
  info->launches = bi.launches + 1;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}
