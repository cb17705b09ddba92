// hsrans_capi_planes_batch.cpp — hsrans_*_device_planes_batch (include/hsrans_hip.h): many tensors' frames of byte planes in one call.  The
// element layer over the batch entries, for K tensors what hsrans_capi_planes.cpp is for one: the workspace layout and the task prefix (pure
// host functions), hsrans_encode_device_planes_batch — one k_planes_split_batch launch, ONE hsrans_encode_device_batch over all planes through
// its public entry, one k_planes_store_batch launch over the planes that did not shrink — and the decode set: ONE hsrans_batch over all coded
// planes, hsrans_decode_device_batch through its public entry and one k_planes_merge_batch launch behind it (hsrans_planes_batch.hip).  The
// kernels' member tables go through the context's task buffers as the gathers' lists do (gather_region_*, hsrans_capi_gather.cpp).
// The two entries' bodies are planes_encode_batch_flow and planes_decode_batch_flow (hsrans_internal.h), which the delta and the diff
// entries below run with a base (or none) per member: then the split and the merge are, by the call's residue rule, the delta or the diff
// kernels (hsrans_planes_base.hip) over the same table with the bases beside it.
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"

#include "hsrans_internal.h"

static_assert(sizeof(hsrans_planes_member) == 240 && sizeof(hsrans_planes_set_info_t) == 32 && sizeof(PlanesBatchMember) == 88, "planes batch ABI and table layout");

namespace
{
constexpr uint32_t kMaxBatchMembers = 65536;  // hsrans_encode_device_batch: members of one call
constexpr uint64_t kMaxBatchTasks = 1u << 24; // ... and fewer mt_ blocks than this

// a member's region of the workspace: hsrans_planes_workspace_bytes, 0 for what that function refuses
size_t region_bytes(uint32_t W, size_t elements) { return hsrans_planes_workspace_bytes(W, elements); }

// Uploads `table` through a region of the context's task buffers and launches `launch(device table)` behind it on `s`, under ctx->lock:
// the gathers' protocol (gather_region_upload).
template <typename Record, typename Launch>
int launch_with_table(hsrans_ctx *ctx, const std::vector<Record> &table, hipStream_t s, Launch &&launch)
{
  std::lock_guard<std::mutex> lk(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  const size_t bytes = table.size() * sizeof(Record);
  return gather_region_upload(
      ctx, bytes, s,
      [&](uint8_t *host) {
        memcpy(host, table.data(), bytes);
        return HSRANS_OK;
      },
      [&](const uint8_t *dev) { return launch((const Record *)dev); });
}

// The split or the merge of a batch: `plain(device table, members, tasks, stream)` over the table as it is, or with d_bases
// `with_base(rule, ...)` over the table of the kernels that take a base (hsrans_planes_base.hip) — the plain records with every member's
// base (null: none).  (Two record types, so two kernels: the choice stays.)
template <typename Plain, typename WithBase>
int launch_split_or_merge(hsrans_ctx *ctx, const std::vector<PlanesBatchMember> &table, const void *const *d_bases, PlanesRule rule, uint32_t n_tasks, hipStream_t s,
                          Plain plain, WithBase with_base)
{
  const uint32_t count = (uint32_t)table.size();
  if (d_bases == nullptr)
    return launch_with_table(ctx, table, s, [&](const PlanesBatchMember *d) { return plain(d, count, n_tasks, s); });
  std::vector<PlanesDeltaBatchMember> with_bases(count);
  for (uint32_t k = 0; k < count; k++)
    with_bases[k] = PlanesDeltaBatchMember{table[k], (const uint8_t *)d_bases[k]};
  return launch_with_table(ctx, with_bases, s, [&](const PlanesDeltaBatchMember *d) { return with_base(rule, d, count, n_tasks, s); });
}

// every output of a failed encode: no frame, no descriptor, no plan (one already made is destroyed)
void fail_encode(hsrans_planes_member *members, uint32_t count, hsrans_dplan **out_dplans, int rc)
{
  for (uint32_t k = 0; k < count; k++)
  {
    members[k].desc = hsrans_planes_desc{};
    members[k].frame_length = 0;
    members[k].rc = rc;
  }
  for (size_t j = 0; out_dplans != nullptr && j < (size_t)count * HSRANS_PLANES_MAX; j++)
    if (out_dplans[j] != nullptr)
    {
      hsrans_dplan_destroy(out_dplans[j]);
      out_dplans[j] = nullptr;
    }
}
} // namespace

extern "C" size_t hsrans_planes_batch_workspace_bytes(const uint32_t *elem_sizes, const size_t *elements, uint32_t count)
{
  if (elem_sizes == nullptr || elements == nullptr || count == 0)
    return 0;
  size_t total = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    // (a member's value is elem_size * up256(elements): it must not wrap either)
    if (elements[k] > (~(size_t)0 - 255) / HSRANS_PLANES_MAX)
      return 0;
    const size_t bytes = region_bytes(elem_sizes[k], elements[k]);
    if (bytes == 0 || total + bytes < total)
      return 0;
    total += bytes;
  }
  return total;
}

extern "C" size_t hsrans_planes_batch_tasks(const size_t *elements, uint32_t count, uint32_t *first_task)
{
  if (elements == nullptr || count == 0)
    return 0;
  uint64_t total = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    if (elements[k] == 0 || elements[k] > kPlanesMaxElements)
      return 0;
    total += planes_tasks_of(elements[k]); // (at most 2^30 each, 2^32 members: no overflow)
  }
  if (total >= 0x80000000u)
    return 0;
  if (first_task != nullptr)
  {
    uint32_t at = 0;
    for (uint32_t k = 0; k < count; k++)
    {
      first_task[k] = at;
      at += planes_tasks_of(elements[k]);
    }
    first_task[count] = at;
  }
  return (size_t)total;
}

int planes_encode_batch_flow(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases, const size_t *base_bytes, bool delta, PlanesRule rule, uint32_t count,
                             void *d_work, size_t work_bytes, void *hip_stream, hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats)
try
{
  if (stats != nullptr)
    *stats = hsrans_planes_batch_stats{};
  if (members == nullptr || count == 0 || count > kMaxBatchMembers)
    return HSRANS_E_ARG;
  for (size_t j = 0; out_dplans != nullptr && j < (size_t)count * HSRANS_PLANES_MAX; j++)
    out_dplans[j] = nullptr; // (the caller's array may hold anything: nothing to destroy yet)
  fail_encode(members, count, out_dplans, HSRANS_OK);
  if (ctx == nullptr || (delta && (d_bases == nullptr || base_bytes == nullptr)))
    return HSRANS_E_ARG;

  // ---- everything checked before anything is launched: each member by its single call's rules, then the call's own ----
  std::vector<PlanesEncShape> shape(count);
  std::vector<size_t> elements(count), work_at(count + 1);
  std::vector<uint32_t> first_task(count + 1);
  bool ok = aligned16(d_work) && !wraps(d_work, work_bytes);
  uint64_t n_planes = 0, n_blocks = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_planes_member &m = members[k];
    if (!planes_encode_check(m.elem_size, m.states, m.bits, m.d_in, m.elements, m.d_frame, m.frame_capacity, m.block_size, m.index_interval, m.flags,
                             out_dplans != nullptr, &shape[k]) ||
        wraps(m.d_in, m.elements * m.elem_size) || wraps(m.d_frame, m.frame_capacity))
    {
      members[k].rc = HSRANS_E_ARG;
      ok = false;
      continue;
    }
    elements[k] = m.elements;
    work_at[k + 1] = work_at[k] + region_bytes(m.elem_size, m.elements); // (elements <= 2^42: no overflow over 65,536 members)
    n_planes += m.elem_size;
    n_blocks += (uint64_t)shape[k].n_blocks * m.elem_size;
  }
  if (!ok)
    return HSRANS_E_ARG;
  const size_t n_tasks = hsrans_planes_batch_tasks(elements.data(), count, first_task.data());
  if (n_planes > kMaxBatchMembers || n_blocks >= kMaxBatchTasks || n_tasks == 0 || work_bytes < work_at[count])
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans;
    spans.reserve(2 * (size_t)count + 1);
    spans.push_back(span_of(d_work, work_bytes, true));
    for (uint32_t k = 0; k < count; k++)
    {
      spans.push_back(span_of(members[k].d_in, members[k].elements * members[k].elem_size, false));
      spans.push_back(span_of(members[k].d_frame, members[k].frame_capacity, true));
      if (delta && d_bases[k] != nullptr && !planes_base_spans(PlanesBase{true, d_bases[k], base_bytes[k]}, members[k].elem_size, members[k].elements, nullptr, 0, &spans))
      {
        members[k].rc = HSRANS_E_ARG;
        return HSRANS_E_ARG;
      }
    }
    if (!spans_disjoint(spans))
      return HSRANS_E_ARG;
  }

  // ---- the split: every member's planes into its region of the workspace ----
  hipStream_t s = (hipStream_t)hip_stream;
  std::vector<PlanesBatchMember> table(count);
  for (uint32_t k = 0; k < count; k++)
  {
    PlanesBatchMember &t = table[k];
    t.elements = (uint8_t *)members[k].d_in;
    for (uint32_t p = 0; p < members[k].elem_size; p++)
      t.plane[p] = (uint8_t *)d_work + work_at[k] + p * shape[k].work_stride;
    t.n = members[k].elements;
    t.W = members[k].elem_size;
    t.first_task = first_task[k];
  }
  int rc = launch_split_or_merge(ctx, table, delta ? d_bases : nullptr, rule, (uint32_t)n_tasks, s, launch_planes_split_batch, launch_planes_split_base_batch);
  if (rc != HSRANS_OK)
  {
    fail_encode(members, count, out_dplans, rc);
    return rc;
  }

  // ---- ONE codec batch over all planes (ctx->lock is not held here: hsrans_encode_device_batch takes it, and it is not recursive) ----
  std::vector<hsrans_encode_member> em((size_t)n_planes);
  std::vector<hsrans_dplan *> plans(out_dplans != nullptr ? (size_t)n_planes : 0, nullptr);
  std::vector<uint32_t> plane_at(count + 1); // member k's planes are em[plane_at[k] ..]
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_planes_member &m = members[k];
    plane_at[k + 1] = plane_at[k] + m.elem_size;
    for (uint32_t p = 0; p < m.elem_size; p++)
    {
      hsrans_encode_member &e = em[plane_at[k] + p];
      e = hsrans_encode_member{};
      e.container = HSRANS_MT;
      e.states = m.states;
      e.bits = m.bits;
      e.block_size = m.block_size;
      e.d_in = table[k].plane[p];
      e.length = m.elements;
      e.d_out = (uint8_t *)m.d_frame + p * shape[k].stride;
      e.out_capacity = shape[k].stride;
      e.index_interval = m.index_interval;
    }
  }
  hsrans_encode_batch_stats es{};
  rc = hsrans_encode_device_batch(ctx, em.data(), (uint32_t)n_planes, hip_stream, out_dplans != nullptr ? plans.data() : nullptr, &es);
  for (uint32_t k = 0; out_dplans != nullptr && k < count; k++) // (handed over first: whatever happens next, the caller's array owns them)
    for (uint32_t p = 0; p < members[k].elem_size; p++)
      out_dplans[(size_t)k * HSRANS_PLANES_MAX + p] = plans[plane_at[k] + p];
  if (rc != HSRANS_OK)
  {
    fail_encode(members, count, out_dplans, rc);
    return rc;
  }

  // ---- the planes that did not shrink: their bytes instead of their streams, one launch for all of them ----
  std::vector<PlanesBatchMember> stores;
  uint64_t store_tasks = 0;
  for (uint32_t k = 0; k < count; k++)
    for (uint32_t p = 0; p < members[k].elem_size; p++)
      if ((members[k].flags & HSRANS_PLANES_STORE_INCOMPRESSIBLE) != 0 && em[plane_at[k] + p].stream_length >= members[k].elements)
      {
        PlanesBatchMember t{};
        t.elements = (uint8_t *)em[plane_at[k] + p].d_out;
        t.plane[0] = table[k].plane[p];
        t.n = members[k].elements;
        t.W = 1;
        t.first_task = (uint32_t)store_tasks;
        store_tasks += planes_tasks_of(t.n); // (up to 8 x the split's: the launch's limit is checked below)
        stores.push_back(t);
      }
  if (!stores.empty())
  {
    rc = store_tasks < 0x80000000u ? launch_with_table(ctx, stores, s, [&](const PlanesBatchMember *d) {
      return launch_planes_store_batch(d, (uint32_t)stores.size(), (uint32_t)store_tasks, s);
    })
                                   : HSRANS_E_ARG;
    if (!stream_settle(s, rc == HSRANS_OK) && rc == HSRANS_OK)
      rc = HSRANS_E_HIP;
    if (rc != HSRANS_OK)
    {
      fail_encode(members, count, out_dplans, rc);
      return rc;
    }
  }

  for (uint32_t k = 0; k < count; k++)
  {
    hsrans_planes_member &m = members[k];
    hsrans_planes_desc &desc = m.desc;
    const uint32_t W = m.elem_size;
    desc.elem_size = W;
    desc.states = (uint32_t)m.states;
    desc.bits = m.bits;
    desc.block_size = m.block_size;
    desc.index_interval = m.index_interval;
    desc.elements = m.elements;
    for (uint32_t p = 0; p < W; p++)
    {
      const size_t length = em[plane_at[k] + p].stream_length;
      const bool is_stored = (m.flags & HSRANS_PLANES_STORE_INCOMPRESSIBLE) != 0 && length >= m.elements;
      desc.stored_mask |= is_stored ? 1u << p : 0;
      desc.offset[p] = p * shape[k].stride;
      desc.length[p] = is_stored ? m.elements : length;
      desc.frame_length = desc.offset[p] + desc.length[p];
      hsrans_dplan **plan = out_dplans != nullptr ? &out_dplans[(size_t)k * HSRANS_PLANES_MAX + p] : nullptr;
      if (is_stored && plan != nullptr && *plan != nullptr)
      {
        hsrans_dplan_destroy(*plan);
        *plan = nullptr;
      }
    }
    m.frame_length = (size_t)desc.frame_length;
    m.rc = HSRANS_OK;
  }
  if (stats != nullptr)
  {
    stats->launches = es.launches + 1 + (stores.empty() ? 0 : 1);
    stats->members = count;
    stats->planes = (uint32_t)n_planes;
    stats->stored = (uint32_t)stores.size();
  }
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI; thrown only after the caller's arrays were reset)
{
  if (members != nullptr && count != 0 && count <= kMaxBatchMembers)
    fail_encode(members, count, out_dplans, HSRANS_E_HIP);
  return HSRANS_E_HIP;
}

extern "C" int hsrans_encode_device_planes_batch(hsrans_ctx *ctx, hsrans_planes_member *members, uint32_t count, void *d_work, size_t work_bytes, void *hip_stream,
                                                 hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats)
{
  return planes_encode_batch_flow(ctx, members, nullptr, nullptr, false, PlanesRule::kXor, count, d_work, work_bytes, hip_stream, out_dplans, stats);
}

extern "C" int hsrans_encode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases, const size_t *base_bytes, uint32_t count,
                                                       void *d_work, size_t work_bytes, void *hip_stream, hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats)
{
  return planes_encode_batch_flow(ctx, members, d_bases, base_bytes, true, PlanesRule::kXor, count, d_work, work_bytes, hip_stream, out_dplans, stats);
}

extern "C" int hsrans_encode_device_planes_diff_batch(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases, const size_t *base_bytes, uint32_t count,
                                                      void *d_work, size_t work_bytes, void *hip_stream, hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats)
{
  return planes_encode_batch_flow(ctx, members, d_bases, base_bytes, true, PlanesRule::kDiff, count, d_work, work_bytes, hip_stream, out_dplans, stats);
}

extern "C" void hsrans_planes_set_destroy(hsrans_planes_set *set)
{
  if (set == nullptr)
    return;
  if (set->batch != nullptr)
    hsrans_dplan_batch_destroy(set->batch);
  delete set;
}

extern "C" int hsrans_planes_set_create(hsrans_ctx *ctx, const hsrans_planes_desc *descs, hsrans_dplan *const *dplans, uint32_t count, hsrans_planes_set **out)
try
{
  if (out == nullptr)
    return HSRANS_E_ARG;
  *out = nullptr;
  if (ctx == nullptr || descs == nullptr || dplans == nullptr || count == 0)
    return HSRANS_E_ARG;
  for (uint32_t k = 0; k < count; k++)
    if (planes_desc_check(ctx, &descs[k], dplans + (size_t)k * HSRANS_PLANES_MAX) != HSRANS_OK)
      return HSRANS_E_ARG;

  hsrans_planes_set *set = new (std::nothrow) hsrans_planes_set;
  if (set == nullptr)
    return HSRANS_E_HIP;
  struct Guard // (an exception on its way to the handler below must not leak the object and its batch)
  {
    hsrans_planes_set *set;
    bool armed = true;
    ~Guard()
    {
      if (armed)
        hsrans_planes_set_destroy(set);
    }
  } guard{set};
  set->ctx = ctx;
  set->descs.assign(descs, descs + count);
  std::vector<size_t> elements(count);
  std::vector<uint32_t> widths(count);
  std::vector<hsrans_dplan *> coded;
  set->work_at.assign(count + 1, 0);
  set->first_task.assign(count + 1, 0);
  for (uint32_t k = 0; k < count; k++)
  {
    elements[k] = (size_t)descs[k].elements;
    widths[k] = descs[k].elem_size;
    set->work_at[k + 1] = set->work_at[k] + region_bytes(widths[k], elements[k]);
    for (uint32_t p = 0; p < widths[k]; p++)
      if (hsrans_dplan *d = dplans[(size_t)k * HSRANS_PLANES_MAX + p])
      {
        coded.push_back(d);
        set->coded_member.push_back(k);
        set->coded_plane.push_back(p);
      }
  }
  // (the size functions refuse what no call could take: an overflow of the workspace, 2^31 tasks or more)
  if (hsrans_planes_batch_workspace_bytes(widths.data(), elements.data(), count) != set->work_at[count] ||
      hsrans_planes_batch_tasks(elements.data(), count, set->first_task.data()) == 0 || coded.size() > 0xFFFFFFFFu)
    return HSRANS_E_ARG;
  set->coded_plans = coded;
  if (!coded.empty())
  {
    const int rc = hsrans_dplan_batch_create(ctx, coded.data(), (uint32_t)coded.size(), &set->batch); // (refuses a plan that appears twice)
    if (rc != HSRANS_OK)
      return rc;
    hsrans_batch_info bi{};
    if (hsrans_dplan_batch_info(set->batch, &bi) != HSRANS_OK)
      return HSRANS_E_HIP;
    set->batch_launches = bi.launches;
  }
  guard.armed = false;
  *out = set;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_set_info(const hsrans_planes_set *set, hsrans_planes_set_info_t *info)
{
  if (set == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  *info = hsrans_planes_set_info_t{};
  info->members = (uint32_t)set->descs.size();
  info->coded = (uint32_t)set->coded_member.size();
  for (const hsrans_planes_desc &d : set->descs)
    info->stored += d.elem_size;
  info->stored -= info->coded;
  info->launches = set->batch_launches + 1;
  info->merge_tasks = set->first_task.back();
  info->work_bytes = set->work_at.back();
  return HSRANS_OK;
}

int planes_decode_batch_flow(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths, const void *const *d_bases,
                             const size_t *base_bytes, bool delta, PlanesRule rule, void *const *d_outs, const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream)
try
{
  if (ctx == nullptr || (delta && (d_bases == nullptr || base_bytes == nullptr)) || set == nullptr || set->ctx != ctx || d_frames == nullptr || frame_lengths == nullptr || d_outs == nullptr || out_capacities == nullptr ||
      !aligned16(d_work) || wraps(d_work, work_bytes) || work_bytes < set->work_at.back())
    return HSRANS_E_ARG;
  const uint32_t count = (uint32_t)set->descs.size();

  // ---- everything checked before anything is launched or uploaded ----
  std::vector<Span> spans, frame_spans, base_spans; // (the last two: a base keeps clear of every member's frame, reads though both are)
  spans.reserve(2 * (size_t)count + 1);
  spans.push_back(span_of(d_work, work_bytes, true));
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_planes_desc &desc = set->descs[k];
    if (!aligned16(d_frames[k]) || !aligned16(d_outs[k]) || frame_lengths[k] < desc.frame_length || out_capacities[k] < desc.elements * desc.elem_size ||
        wraps(d_frames[k], frame_lengths[k]) || wraps(d_outs[k], out_capacities[k]))
      return HSRANS_E_ARG;
    spans.push_back(span_of(d_frames[k], frame_lengths[k], false));
    spans.push_back(span_of(d_outs[k], out_capacities[k], true));
    if (delta && d_bases[k] != nullptr &&
        !planes_base_spans(PlanesBase{true, d_bases[k], base_bytes[k]}, desc.elem_size, (size_t)desc.elements, d_outs[k], out_capacities[k], &spans))
      return HSRANS_E_ARG;
    if (delta)
      frame_spans.push_back(span_of(d_frames[k], frame_lengths[k], false));
    if (delta && d_bases[k] != nullptr)
      base_spans.push_back(span_of(d_bases[k], base_bytes[k], false));
  }
  if (!spans_disjoint(spans) || spans_meet(base_spans, frame_spans))
    return HSRANS_E_ARG;

  // ---- the merge's sources: a coded plane decoded into its member's region of the workspace, a stored one where it lies in its frame ----
  std::vector<PlanesBatchMember> table(count);
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_planes_desc &desc = set->descs[k];
    PlanesBatchMember &t = table[k];
    t.elements = (uint8_t *)d_outs[k];
    for (uint32_t p = 0; p < desc.elem_size; p++)
      t.plane[p] = (desc.stored_mask >> p) & 1 ? (uint8_t *)d_frames[k] + desc.offset[p] : (uint8_t *)d_work + set->work_at[k] + p * up256((size_t)desc.elements);
    t.n = desc.elements;
    t.W = desc.elem_size;
    t.first_task = set->first_task[k];
  }
  if (set->batch != nullptr)
  {
    const size_t coded = set->coded_member.size();
    std::vector<const void *> streams(coded);
    std::vector<void *> outs(coded);
    std::vector<size_t> lengths(coded), caps(coded);
    for (size_t j = 0; j < coded; j++)
    {
      const uint32_t k = set->coded_member[j], p = set->coded_plane[j];
      streams[j] = (const uint8_t *)d_frames[k] + set->descs[k].offset[p];
      lengths[j] = (size_t)set->descs[k].length[p];
      outs[j] = table[k].plane[p];
      caps[j] = (size_t)set->descs[k].elements;
    }
    const int rc = hsrans_decode_device_batch(ctx, set->batch, streams.data(), lengths.data(), outs.data(), caps.data(), hip_stream);
    if (rc != HSRANS_OK)
      return rc;
  }
  return launch_split_or_merge(ctx, table, delta ? d_bases : nullptr, rule, set->first_task.back(), (hipStream_t)hip_stream, launch_planes_merge_batch,
                               launch_planes_merge_base_batch);
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_decode_device_planes_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths, void *const *d_outs,
                                                 const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_decode_batch_flow(ctx, set, d_frames, frame_lengths, nullptr, nullptr, false, PlanesRule::kXor, d_outs, out_capacities, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                                       const void *const *d_bases, const size_t *base_bytes, void *const *d_outs, const size_t *out_capacities, void *d_work,
                                                       size_t work_bytes, void *hip_stream)
{
  return planes_decode_batch_flow(ctx, set, d_frames, frame_lengths, d_bases, base_bytes, true, PlanesRule::kXor, d_outs, out_capacities, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_decode_device_planes_diff_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                                      const void *const *d_bases, const size_t *base_bytes, void *const *d_outs, const size_t *out_capacities, void *d_work,
                                                      size_t work_bytes, void *hip_stream)
{
  return planes_decode_batch_flow(ctx, set, d_frames, frame_lengths, d_bases, base_bytes, true, PlanesRule::kDiff, d_outs, out_capacities, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_planes_set_status(hsrans_ctx *ctx, hsrans_planes_set *set, void *hip_stream, int *member_status)
try
{
  if (ctx == nullptr || set == nullptr || set->ctx != ctx)
    return HSRANS_E_ARG;
  for (size_t k = 0; member_status != nullptr && k < set->descs.size(); k++)
    member_status[k] = HSRANS_OK;
  if (set->batch == nullptr) // (every plane stored: nothing to report, but the call still waits for the stream as the batch's does)
    return hipSetDevice(ctx->device) == hipSuccess && stream_settle((hipStream_t)hip_stream, true) ? HSRANS_OK : HSRANS_E_HIP;
  std::vector<int> plane_status(set->coded_member.size(), HSRANS_OK);
  const int rc = hsrans_dplan_batch_status(ctx, set->batch, hip_stream, plane_status.data());
  for (size_t j = 0; member_status != nullptr && j < plane_status.size(); j++)
    if (plane_status[j] != HSRANS_OK && member_status[set->coded_member[j]] == HSRANS_OK)
      member_status[set->coded_member[j]] = plane_status[j];
  return rc;
}
catch (...)
{
  return HSRANS_E_HIP;
}
