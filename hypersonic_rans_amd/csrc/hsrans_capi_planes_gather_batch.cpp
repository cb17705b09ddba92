// hsrans_capi_planes_gather_batch.cpp — hsrans_decode_device_planes_gather_batch (include/hsrans_hip.h): element ranges of MANY frames of
// byte planes in one call.  For K tensors what hsrans_capi_planes_gather.cpp is for one: the object (a hsrans_planes_set bound to its
// frames, ONE hsrans_gather_set over all coded planes of all members, one record per member in device memory for the merge), the workspace
// layout for rows of mixed element sizes and the host-side cut of the merge (hsrans_planes_gather_batch_tasks, a pure function on the rules
// of planes_cut.h), the argument checks, and the call: hsrans_decode_device_gather_batch of the coded planes' bytes into the workspace
// through its public entry, then one k_planes_merge_ranges_batch launch (hsrans_planes_gather_batch.hip) whose task list goes through the
// context's task buffer as the gathers' lists do (gather_region_*, hsrans_capi_gather.cpp).
// hsrans_decode_device_planes_gather_batch_indirect, at the end of the file: the same for rows in device memory — the device cuts
// (hsrans_planes_gather_batch_indirect.hip), by the rules of planes_cut_batch.h that measure_rows above uses too.
// Both calls' bodies are flows (planes_gather_batch_flow, planes_gather_batch_indirect_flow: hsrans_internal.h) that take an optional
// hsrans_planes_base_set, defined here too: with one they are hsrans_decode_device_planes_gather_batch_delta and
// hsrans_decode_device_planes_gather_batch_indirect_delta, whose merges XOR each member's base in (hsrans_planes_gather_delta.hip).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_planes.h"
#include "planes_cut_batch.h"

#include "hsrans_internal.h"

static_assert(sizeof(hsrans_planes_gather_batch_task) == 48 && sizeof(PlanesGatherBatchTask) == sizeof(hsrans_planes_gather_batch_task) &&
                  sizeof(hsrans_member_range) == 32 && sizeof(hsrans_planes_gather_set_info_t) == 24,
              "planes gather batch ABI layout");

struct hsrans_planes_gather_set
{
  hsrans_ctx *ctx = nullptr;
  hsrans_planes_set *planes = nullptr;
  hsrans_gather_set *set = nullptr; // over the coded planes of all members, in the planes set's coded order; null when every plane is stored
  std::vector<uint32_t> widths;     // per member: elem_size ...
  std::vector<uint64_t> elements;   // ... elements ...
  std::vector<uint32_t> coded_mask; // ... which planes are coded ...
  std::vector<uint32_t> coded_at;   // [members + 1] ... and where its coded planes begin among the set's members
  std::vector<Span> frames;         // the frames over frame_lengths, sorted by address
  PlanesGatherBatchMember *d_members = nullptr; // the merge's records, uploaded once
  PlanesCutBatchMember *d_cut_members = nullptr; // ... and what k_planes_cut_batch reads of a member (hsrans_decode_device_planes_gather_batch_indirect)
  uint32_t min_width = 0, max_width = 0;         // the smallest and the largest element size among the members
  uint32_t *d_refused = nullptr; // the object's own status word (kStatusBadRange: k_planes_cut_batch refused an indirect call); no plan's word is involved
  hsrans_planes_gather_set_info_t last{};       // members, coded, stored; the last call's part (under ctx->lock)
};

namespace
{
static_assert(kPlanesCutTask == kPlanesGatherTaskElements, "planes_cut.h cuts at the merge kernels' task length");

// What the rows come to: the merge's tasks, the workspace's bytes (the sum of W * slot) and, with `coded_at`, the rows of the set's gather
struct BatchCut
{
  uint64_t tasks = 0, work = 0, rows = 0;
};
// whether every row names a member, lies inside it and leaves every total in range (tasks and gather rows below 2^31, a launch's workgroups
// and the set's limit; no sum wraps)
bool measure_rows(const hsrans_member_range *ranges, uint32_t count, const uint32_t *elem_sizes, const uint64_t *elements, uint32_t members, const uint32_t *coded_at,
                  BatchCut *cut)
{
  *cut = BatchCut{};
  PlanesRowsSum sum{0, 0, 0};
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_member_range &g = ranges[r];
    PlanesRowCut row;
    if (g.member >= members || g.reserved != 0 ||
        !planes_row_cut(g.offset, g.length, elements[g.member], elem_sizes[g.member], coded_at != nullptr ? coded_at[g.member + 1] - coded_at[g.member] : 0, &row) ||
        !planes_rows_add(&sum, row))
      return false;
  }
  *cut = BatchCut{sum.tasks, sum.work, sum.rows};
  return true;
}

// The cut of the merge for rows that passed measure_rows: task(record) for every task, in row order.  Slot, task count and task k of a row
// are planes_cut.h's with the row's base C_r; the row's sub-slots lie slot_r apart.
template <typename Task>
void cut_rows(const hsrans_member_range *ranges, uint32_t count, const uint32_t *elem_sizes, Task &&task)
{
  uint64_t at = 0; // C_r
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_member_range &g = ranges[r];
    const uint64_t slot = planes_range_slot(g.offset, g.length);
    for (uint64_t k = 0, n = planes_range_tasks(g.offset, g.length); k < n; k++)
    {
      const hsrans_planes_gather_task t = planes_task_at<hsrans_planes_gather_task>(g.offset, g.length, g.dst_offset, at, k);
      task(hsrans_planes_gather_batch_task{t.src, t.work_pos, slot, t.dst_delta, t.lo, t.hi, g.member, 0});
    }
    at += elem_sizes[g.member] * slot;
  }
}
} // namespace

extern "C" size_t hsrans_planes_gather_batch_workspace_bytes(uint32_t max_elem_size, uint32_t count, uint64_t total_elements)
{
  const uint64_t bytes = total_elements + 30 * (uint64_t)count;
  if (!planes_width_ok(max_elem_size) || bytes < total_elements || bytes > (~(uint64_t)0 - 255) / max_elem_size)
    return 0;
  return up256((size_t)(max_elem_size * bytes));
}

extern "C" size_t hsrans_planes_gather_batch_tasks(const hsrans_member_range *ranges, uint32_t count, const uint32_t *elem_sizes, const uint64_t *elements, uint32_t members,
                                                   hsrans_planes_gather_batch_task *out, size_t capacity)
{
  BatchCut cut;
  if ((ranges == nullptr && count > 0) || ((elem_sizes == nullptr || elements == nullptr) && members > 0) || (out == nullptr && capacity > 0) ||
      !measure_rows(ranges, count, elem_sizes, elements, members, nullptr, &cut))
    return 0;
  if (capacity == 0) // (the count alone: no walk over up to 2^31 tasks)
    return (size_t)cut.tasks;
  size_t n = 0;
  cut_rows(ranges, count, elem_sizes, [&](const hsrans_planes_gather_batch_task &t) {
    if (n < capacity)
      out[n] = t;
    n++;
  });
  return n;
}

extern "C" void hsrans_planes_gather_set_destroy(hsrans_planes_gather_set *pgs)
{
  if (pgs == nullptr)
    return;
  if (pgs->set != nullptr)
    hsrans_gather_set_destroy(pgs->set);
  if (pgs->d_members != nullptr)
    (void)hipFree(pgs->d_members);
  if (pgs->d_cut_members != nullptr)
    (void)hipFree(pgs->d_cut_members);
  if (pgs->d_refused != nullptr)
    (void)hipFree(pgs->d_refused);
  delete pgs;
}

extern "C" int hsrans_planes_gather_set_create(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths, hsrans_planes_gather_set **out)
try
{
  if (out == nullptr)
    return HSRANS_E_ARG;
  *out = nullptr;
  if (ctx == nullptr || set == nullptr || set->ctx != ctx || d_frames == nullptr || frame_lengths == nullptr)
    return HSRANS_E_ARG;
  const uint32_t members = (uint32_t)set->descs.size();
  for (uint32_t k = 0; k < members; k++)
    if (!aligned16(d_frames[k]) || frame_lengths[k] < set->descs[k].frame_length || wraps(d_frames[k], frame_lengths[k]))
      return HSRANS_E_ARG;

  hsrans_planes_gather_set *pgs = new (std::nothrow) hsrans_planes_gather_set;
  if (pgs == nullptr)
    return HSRANS_E_HIP;
  struct Guard // (an exception on its way to the handler below must not leak the object, its set and its records)
  {
    hsrans_planes_gather_set *pgs;
    bool armed = true;
    ~Guard()
    {
      if (armed)
        hsrans_planes_gather_set_destroy(pgs);
    }
  } guard{pgs};
  pgs->ctx = ctx;
  pgs->planes = set;
  pgs->coded_at.assign(members + 1, 0);
  std::vector<PlanesGatherBatchMember> records(members);
  std::vector<PlanesCutBatchMember> cut_records(std::max(members, 1u)); // (never empty: the cut reads record 0 for a member beyond the set's)
  for (uint32_t k = 0; k < members; k++)
  {
    const hsrans_planes_desc &desc = set->descs[k];
    const uint32_t all = (1u << desc.elem_size) - 1, mask = all & ~desc.stored_mask;
    pgs->widths.push_back(desc.elem_size);
    pgs->elements.push_back(desc.elements);
    pgs->coded_mask.push_back(mask);
    pgs->coded_at[k + 1] = pgs->coded_at[k] + (uint32_t)__builtin_popcount(mask);
    pgs->frames.push_back(span_of(d_frames[k], frame_lengths[k], false));
    records[k].W = desc.elem_size;
    records[k].coded_mask = mask;
    for (uint32_t p = 0; p < desc.elem_size; p++)
      records[k].stored[p] = (mask >> p) & 1 ? nullptr : (const uint8_t *)d_frames[k] + desc.offset[p];
    cut_records[k] = PlanesCutBatchMember{desc.elements, pgs->coded_at[k], (uint16_t)desc.elem_size, (uint16_t)mask};
    pgs->min_width = k == 0 ? desc.elem_size : std::min(pgs->min_width, desc.elem_size);
    pgs->max_width = std::max(pgs->max_width, desc.elem_size);
  }
  const size_t coded = set->coded_plans.size();
  if (pgs->coded_at[members] != coded) // (the planes set lists exactly the planes its descriptors call coded, in member and plane order)
    return HSRANS_E_ARG;
  std::sort(pgs->frames.begin(), pgs->frames.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; }); // (a call's spans_disjoint finds them sorted)
  pgs->last.members = members;
  pgs->last.coded = (uint32_t)coded;
  pgs->last.stored = 0;
  for (uint32_t k = 0; k < members; k++)
    pgs->last.stored += pgs->widths[k];
  pgs->last.stored -= pgs->last.coded;

  if (coded != 0)
  {
    if (coded > 0xFFFFFFFFu)
      return HSRANS_E_ARG;
    std::vector<const void *> streams(coded);
    std::vector<size_t> lengths(coded);
    for (size_t j = 0; j < coded; j++)
    {
      const uint32_t k = set->coded_member[j], p = set->coded_plane[j];
      streams[j] = (const uint8_t *)d_frames[k] + set->descs[k].offset[p];
      lengths[j] = (size_t)set->descs[k].length[p];
    }
    const int rc = hsrans_gather_set_create(ctx, set->coded_plans.data(), streams.data(), lengths.data(), (uint32_t)coded, &pgs->set); // (E_ARG beyond 65,536)
    if (rc != HSRANS_OK)
      return rc;
  }
  // the merge's records and the cut's, once (as hsrans_gather_set_create uploads the set's), and the word the indirect call's cut reports a
  // refusal in
  const size_t bytes = records.size() * sizeof(PlanesGatherBatchMember), cut_bytes = cut_records.size() * sizeof(PlanesCutBatchMember);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)&pgs->d_members, bytes) != hipSuccess ||
      hipMemcpy(pgs->d_members, records.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMalloc((void **)&pgs->d_cut_members, cut_bytes) != hipSuccess ||
      hipMemcpy(pgs->d_cut_members, cut_records.data(), cut_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      refusal_word_create(ctx, &pgs->d_refused) != HSRANS_OK)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  guard.armed = false;
  *out = pgs;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_planes_base_set: one base per member of a gather set, for the delta forms of the two calls below.  The addresses are uploaded
// once, one uint64 per member (0: the member goes as it is), so that the device-rows call stays kernels and nothing else; the host keeps
// the bases' spans for the calls' overlap checks.  Neither the gather set nor the planes set is touched.
// ---------------------------------------------------------------------------------------------------------------
struct hsrans_planes_base_set
{
  hsrans_ctx *ctx = nullptr;
  hsrans_planes_gather_set *pgs = nullptr;
  std::vector<Span> bases;      // the members' bases over base_bytes, those that are set: read spans
  uint64_t *d_xbases = nullptr; // [members]: what the delta merges read
};

extern "C" void hsrans_planes_base_set_destroy(hsrans_planes_base_set *bs)
{
  if (bs == nullptr)
    return;
  if (bs->d_xbases != nullptr)
    (void)hipFree(bs->d_xbases);
  delete bs;
}

extern "C" int hsrans_planes_base_set_create(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const void *const *d_bases, const size_t *base_bytes, hsrans_planes_base_set **out)
try
{
  if (out == nullptr)
    return HSRANS_E_ARG;
  *out = nullptr;
  if (ctx == nullptr || pgs == nullptr || pgs->ctx != ctx || d_bases == nullptr || base_bytes == nullptr)
    return HSRANS_E_ARG;
  const uint32_t members = (uint32_t)pgs->widths.size();
  std::vector<Span> bases;
  std::vector<uint64_t> table(std::max(members, 1u), 0);
  for (uint32_t k = 0; k < members; k++)
  {
    if (d_bases[k] == nullptr)
      continue;
    std::vector<Span> one;
    if (!planes_base_spans(PlanesBase{true, d_bases[k], base_bytes[k]}, pgs->widths[k], (size_t)pgs->elements[k], nullptr, 0, &one))
      return HSRANS_E_ARG;
    bases.push_back(one[0]);
    table[k] = (uint64_t)(uintptr_t)d_bases[k];
  }
  {
    std::vector<Span> frames(pgs->frames); // (a base over compressed bytes is never a meaningful call, reads though both are)
    if (spans_meet(bases, frames))
      return HSRANS_E_ARG;
  }
  hsrans_planes_base_set *bs = new (std::nothrow) hsrans_planes_base_set;
  if (bs == nullptr)
    return HSRANS_E_HIP;
  bs->ctx = ctx;
  bs->pgs = pgs;
  bs->bases.swap(bases);
  const size_t bytes = table.size() * sizeof(uint64_t);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)&bs->d_xbases, bytes) != hipSuccess ||
      hipMemcpy(bs->d_xbases, table.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
  {
    (void)hipGetLastError();
    hsrans_planes_base_set_destroy(bs);
    return HSRANS_E_HIP;
  }
  *out = bs;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

namespace
{
// A call's base set: none (the plain call), or one of this gather set and context.  Its bases join *spans as reads — they may coincide with
// one another and may not meet anything the call writes (spans_disjoint, the caller's next step)
bool base_set_spans(const hsrans_ctx *ctx, const hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs, std::vector<Span> *spans)
{
  if (bs == nullptr)
    return true;
  if (bs->ctx != ctx || bs->pgs != pgs)
    return false;
  spans->insert(spans->end(), bs->bases.begin(), bs->bases.end());
  return true;
}
} // namespace

// hsrans_decode_device_planes_gather_batch's whole body, and with a base set hsrans_decode_device_planes_gather_batch_delta's: the bases join
// the overlap rule and the merge is k_planes_merge_ranges_batch_delta (hsrans_planes_gather_delta.hip)
int planes_gather_batch_flow(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs, const hsrans_member_range *ranges, uint32_t count, void *d_out,
                             size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
try
{
  if (ctx == nullptr || pgs == nullptr || pgs->ctx != ctx || !aligned16(d_out) || !aligned16(d_work) || (ranges == nullptr && count > 0) || wraps(d_out, out_capacity) ||
      wraps(d_work, work_bytes))
    return HSRANS_E_ARG;
  const uint32_t members = (uint32_t)pgs->widths.size();

  // ---- everything checked before anything is launched or uploaded ----
  BatchCut cut; // (measure_rows is what hsrans_planes_gather_batch_tasks refuses by; here it counts the set's rows too)
  if (!measure_rows(ranges, count, pgs->widths.data(), pgs->elements.data(), members, pgs->coded_at.data(), &cut))
    return HSRANS_E_ARG;
  for (uint32_t r = 0; r < count; r++)
    if (!planes_dest_ok(ranges[r].dst_offset, ranges[r].length, out_capacity / pgs->widths[ranges[r].member]))
      return HSRANS_E_ARG;
  if (cut.work > ~(uint64_t)0 - 255)
    return HSRANS_E_ARG;
  const size_t need = up256((size_t)cut.work); // what this call's layout takes
  if (work_bytes < need)
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans;
    spans.reserve(pgs->frames.size() + 2);
    spans.assign(pgs->frames.begin(), pgs->frames.end());
    spans.push_back(span_of(d_out, out_capacity, true));
    spans.push_back(span_of(d_work, work_bytes, true));
    if (!base_set_spans(ctx, pgs, bs, &spans) || !spans_disjoint(spans))
      return HSRANS_E_ARG;
  }
  {
    std::lock_guard<std::mutex> lk(ctx->lock);
    pgs->last.rows = pgs->last.merge_tasks = pgs->last.launches = 0;
  }
  if (cut.tasks == 0)
    return HSRANS_OK;

  // ---- the coded planes' bytes into their sub-slots: every non-empty row gives one gather row per coded plane of its member, to
  // C_r + p * slot_r + phase ----
  uint32_t set_launches = 0;
  if (cut.rows != 0)
  {
    std::vector<hsrans_member_range> rows;
    rows.reserve((size_t)cut.rows);
    uint64_t at = 0;
    for (uint32_t r = 0; r < count; r++)
    {
      const hsrans_member_range &g = ranges[r];
      if (g.length == 0)
        continue;
      const uint64_t slot = planes_range_slot(g.offset, g.length), phase = g.offset & 15;
      uint32_t j = pgs->coded_at[g.member];
      for (uint32_t p = 0, mask = pgs->coded_mask[g.member]; (mask >> p) != 0; p++)
        if ((mask >> p) & 1)
          rows.push_back(hsrans_member_range{g.offset, g.length, at + p * slot + phase, j++, 0});
      at += pgs->widths[g.member] * slot;
    }
    // (ctx->lock is not held here: hsrans_decode_device_gather_batch takes it, and it is not recursive)
    const int rc = hsrans_decode_device_gather_batch(ctx, pgs->set, rows.data(), (uint32_t)rows.size(), d_work, need, hip_stream);
    if (rc != HSRANS_OK)
      return rc;
    hsrans_gather_set_info_t si{};
    if (hsrans_gather_set_info(pgs->set, &si) != HSRANS_OK)
      return HSRANS_E_HIP;
    set_launches = si.launches;
  }

  // ---- the merge behind it: its task list through the context's task buffer, ordered with the context's gathers ----
  std::lock_guard<std::mutex> lk(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  const int rc = gather_region_upload(
      ctx, (size_t)cut.tasks * sizeof(PlanesGatherBatchTask), s,
      [&](uint8_t *host) {
        hsrans_planes_gather_batch_task *list = (hsrans_planes_gather_batch_task *)host;
        cut_rows(ranges, count, pgs->widths.data(), [&](const hsrans_planes_gather_batch_task &t) { *list++ = t; });
        return HSRANS_OK;
      },
      [&](const uint8_t *dev) {
        const PlanesGatherBatchTask *tasks = (const PlanesGatherBatchTask *)dev;
        return bs != nullptr ? launch_planes_merge_ranges_batch_delta(tasks, (uint32_t)cut.tasks, pgs->d_members, bs->d_xbases, d_work, d_out, s)
                             : launch_planes_merge_ranges_batch(tasks, (uint32_t)cut.tasks, pgs->d_members, d_work, d_out, s);
      });
  if (rc != HSRANS_OK)
    return rc;
  pgs->last.rows = (uint32_t)cut.rows;
  pgs->last.merge_tasks = (uint32_t)cut.tasks;
  pgs->last.launches = set_launches + 1;
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_decode_device_planes_gather_batch(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_member_range *ranges, uint32_t count, void *d_out,
                                                        size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return planes_gather_batch_flow(ctx, pgs, nullptr, ranges, count, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

// (a NULL base set is refused here: the flow reads one as "no bases")
extern "C" int hsrans_decode_device_planes_gather_batch_delta(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs, const hsrans_member_range *ranges,
                                                              uint32_t count, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream)
{
  return bs == nullptr ? HSRANS_E_ARG : planes_gather_batch_flow(ctx, pgs, bs, ranges, count, d_out, out_capacity, d_work, work_bytes, hip_stream);
}

extern "C" int hsrans_planes_gather_set_status(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, void *hip_stream, int *member_status)
try
{
  if (ctx == nullptr || pgs == nullptr || pgs->ctx != ctx)
    return HSRANS_E_ARG;
  for (size_t k = 0; member_status != nullptr && k < pgs->widths.size(); k++)
    member_status[k] = HSRANS_OK;
  if (pgs->set == nullptr)
    return planes_all_stored_status(ctx, hip_stream);
  const std::vector<uint32_t> &coded_member = pgs->planes->coded_member;
  std::vector<int> plane_status(coded_member.size(), HSRANS_OK);
  const int rc = hsrans_gather_set_status(ctx, pgs->set, hip_stream, plane_status.data());
  for (size_t j = 0; member_status != nullptr && j < plane_status.size(); j++)
    if (plane_status[j] != HSRANS_OK && member_status[coded_member[j]] == HSRANS_OK)
      member_status[coded_member[j]] = plane_status[j];
  return rc;
}
catch (...)
{
  return HSRANS_E_HIP;
}

extern "C" int hsrans_planes_gather_set_info(const hsrans_planes_gather_set *pgs, hsrans_planes_gather_set_info_t *info)
{
  if (pgs == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  std::lock_guard<std::mutex> lk(pgs->ctx->lock);
  *info = pgs->last;
  return HSRANS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_planes_gather_batch_indirect: the rows are in device memory.  Nothing of the above is cut here: k_planes_cut_batch
// checks the rows against their members, lays out the workspace and writes the set's rows, the set's indirect entry gathers the coded planes'
// bytes, k_planes_merge_batch_indirect derives its tasks from what the cut left (hsrans_planes_gather_batch_indirect.hip).  No lock, no task
// buffer, no allocation: kernels and nothing else.
// ---------------------------------------------------------------------------------------------------------------
namespace
{
static_assert(sizeof(PlanesSetRow) == sizeof(hsrans_member_range) && sizeof(hsrans_planes_gather_set_indirect_info_t) == 28, "the device's view of the rows; the info's layout");

constexpr uint64_t kWorkLimitMax = (uint64_t)1 << 48; // beyond any device's memory; up to it no sum of W * slot in k_planes_cut_batch can wrap

// What one indirect call launches, from what the host knows: the entry and hsrans_planes_gather_set_indirect_info both go through here.
struct BatchIndirectShape
{
  uint32_t max_rows, merge_grid, set_launches, launches;
};
bool batch_indirect_shape(const hsrans_planes_gather_set *pgs, uint32_t max_count, size_t work_bytes, BatchIndirectShape *shape)
{
  *shape = BatchIndirectShape{};
  const uint32_t coded = pgs->last.coded;
  if (hsrans_planes_gather_batch_indirect_workspace_bytes(coded, pgs->max_width, max_count) == 0) // (no member, or max_count * max_width >= 2^31)
    return false;
  if (max_count == 0)
    return true;
  shape->max_rows = pgs->set != nullptr ? max_count * pgs->max_width : 0;
  shape->merge_grid = planes_merge_batch_indirect_grid(pgs->ctx->geom.num_cus, pgs->min_width, max_count, work_bytes);
  if (pgs->set != nullptr)
  {
    hsrans_gather_set_info_t si{};
    if (hsrans_gather_set_indirect_info(pgs->set, shape->max_rows, work_bytes, &si) != HSRANS_OK)
      return false;
    shape->set_launches = si.launches + 1; // (+ the set's cut)
  }
  shape->launches = shape->set_launches + 2; // (+ k_planes_cut_batch and the merge)
  return true;
}
} // namespace

extern "C" size_t hsrans_planes_gather_batch_indirect_workspace_bytes(uint32_t coded_planes, uint32_t max_elem_size, uint32_t max_count)
{
  if (!planes_width_ok(max_elem_size) || coded_planes > 65536 || (uint64_t)max_count * max_elem_size >= 0x80000000u)
    return 0;
  const size_t control = planes_cut_batch_ws(max_elem_size, max_count).set;
  if (coded_planes == 0) // (every plane stored: no set, no call of its own)
    return control;
  const size_t set_bytes = hsrans_gather_batch_workspace_bytes(coded_planes, max_count * max_elem_size);
  return set_bytes == 0 ? 0 : control + up256(set_bytes);
}

extern "C" int hsrans_planes_gather_set_indirect_info(const hsrans_planes_gather_set *pgs, uint32_t max_count, size_t out_capacity, size_t work_bytes,
                                                      hsrans_planes_gather_set_indirect_info_t *info)
try
{
  if (pgs == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  BatchIndirectShape shape{};
  if (!batch_indirect_shape(pgs, max_count, work_bytes, &shape))
    return HSRANS_E_ARG;
  (void)out_capacity; // (it bounds the destinations on the device; no launch is shaped by it)
  *info = hsrans_planes_gather_set_indirect_info_t{pgs->last.members, pgs->last.coded, pgs->last.stored, shape.max_rows, shape.merge_grid, shape.launches, shape.set_launches};
  return HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}

// the entry's whole body, and with a base set hsrans_decode_device_planes_gather_batch_indirect_delta's: the bases join the overlap rule,
// keep clear of the rows and the count word too, and the merge is k_planes_merge_batch_indirect_delta on its own grid
int planes_gather_batch_indirect_flow(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs, const hsrans_member_range *d_ranges,
                                      const uint32_t *d_count, uint32_t max_count, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace,
                                      size_t workspace_bytes, void *hip_stream)
try
{
  if (ctx == nullptr || pgs == nullptr || pgs->ctx != ctx || d_ranges == nullptr || d_workspace == nullptr || !aligned16(d_out) || !aligned16(d_work))
    return HSRANS_E_ARG;
  if (((uintptr_t)d_ranges & 7) != 0 || ((uintptr_t)d_count & 3) != 0 || ((uintptr_t)d_workspace & 255) != 0)
    return HSRANS_E_ARG;
  const size_t need_ws = hsrans_planes_gather_batch_indirect_workspace_bytes(pgs->last.coded, pgs->max_width, max_count);
  if (need_ws == 0 || workspace_bytes < need_ws || wraps(d_out, out_capacity) || wraps(d_work, work_bytes) || wraps(d_workspace, workspace_bytes))
    return HSRANS_E_ARG;
  {
    std::vector<Span> spans;
    spans.reserve(pgs->frames.size() + 5);
    spans.assign(pgs->frames.begin(), pgs->frames.end());
    spans.push_back(span_of(d_ranges, (size_t)max_count * sizeof(hsrans_member_range), false));
    if (d_count != nullptr)
      spans.push_back(span_of(d_count, sizeof(uint32_t), false));
    spans.push_back(span_of(d_out, out_capacity, true));
    spans.push_back(span_of(d_work, work_bytes, true));
    spans.push_back(span_of(d_workspace, workspace_bytes, true));
    if (!base_set_spans(ctx, pgs, bs, &spans) || !spans_disjoint(spans))
      return HSRANS_E_ARG;
    if (bs != nullptr) // (the rows and the count word are only read, as a base is, and a base over them is no more meaningful than one over a frame)
    {
      std::vector<Span> inputs{span_of(d_ranges, (size_t)max_count * sizeof(hsrans_member_range), false), span_of(d_count, d_count != nullptr ? sizeof(uint32_t) : 0, false)};
      if (spans_meet(bs->bases, inputs))
        return HSRANS_E_ARG;
    }
  }
  if (max_count == 0)
    return HSRANS_OK;
  BatchIndirectShape shape{};
  if (!batch_indirect_shape(pgs, max_count, work_bytes, &shape))
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;

  // ---- the cut: C_r, the task prefix and the set's rows into the control workspace ----
  const PlanesCutBatchWs ws = planes_cut_batch_ws(pgs->max_width, max_count);
  uint8_t *const control = (uint8_t *)d_workspace;
  PlanesCutBatchParams cp{};
  cp.ranges = (const PlanesSetRow *)d_ranges;
  cp.count = d_count;
  cp.members = pgs->d_cut_members;
  cp.max_count = max_count;
  cp.n_members = (uint32_t)pgs->widths.size();
  cp.out_capacity = out_capacity;
  cp.work_limit = std::min<uint64_t>((uint64_t)work_bytes & ~(uint64_t)255, kWorkLimitMax); // (up256(sum) <= work_bytes)
  cp.header = (uint32_t *)control;
  cp.first_task = (uint32_t *)(control + ws.first_task);
  cp.base = (uint64_t *)(control + ws.base);
  cp.first_row = (uint32_t *)(control + ws.first_row);
  cp.rows = (PlanesSetRow *)(control + ws.rows);
  cp.status = pgs->d_refused;
  if (launch_planes_cut_batch(cp, s) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }

  // ---- the coded planes' bytes into their sub-slots, through the set's public entry as the host-rows call goes through the batch entry ----
  if (pgs->set != nullptr)
  {
    const int rc = hsrans_decode_device_gather_batch_indirect(ctx, pgs->set, (const hsrans_member_range *)cp.rows, cp.header + kPlanesWsRows, shape.max_rows, d_work, work_bytes,
                                                              control + ws.set, workspace_bytes - ws.set, hip_stream);
    if (rc != HSRANS_OK)
      return rc;
  }

  // ---- the merge behind it ----
  const hipError_t merged =
      bs != nullptr ? launch_planes_merge_batch_indirect_delta(cp.ranges, cp.header, cp.first_task, cp.base, pgs->d_members, bs->d_xbases, d_work, d_out,
                                                               planes_merge_batch_indirect_delta_grid(ctx->geom.num_cus, pgs->min_width, max_count, work_bytes), s)
                    : launch_planes_merge_batch_indirect(cp.ranges, cp.header, cp.first_task, cp.base, pgs->d_members, d_work, d_out, shape.merge_grid, s);
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

extern "C" int hsrans_decode_device_planes_gather_batch_indirect(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_member_range *d_ranges, const uint32_t *d_count,
                                                                 uint32_t max_count, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace,
                                                                 size_t workspace_bytes, void *hip_stream)
{
  return planes_gather_batch_indirect_flow(ctx, pgs, nullptr, d_ranges, d_count, max_count, d_out, out_capacity, d_work, work_bytes, d_workspace, workspace_bytes, hip_stream);
}

// (a NULL base set is refused here: the flow reads one as "no bases")
extern "C" int hsrans_decode_device_planes_gather_batch_indirect_delta(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs,
                                                                       const hsrans_member_range *d_ranges, const uint32_t *d_count, uint32_t max_count, void *d_out,
                                                                       size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes,
                                                                       void *hip_stream)
{
  return bs == nullptr ? HSRANS_E_ARG
                       : planes_gather_batch_indirect_flow(ctx, pgs, bs, d_ranges, d_count, max_count, d_out, out_capacity, d_work, work_bytes, d_workspace, workspace_bytes,
                                                           hip_stream);
}

extern "C" int hsrans_planes_gather_set_refused(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, void *hip_stream)
try
{
  if (ctx == nullptr || pgs == nullptr || pgs->ctx != ctx)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  const int rc = refusal_word_take(pgs->d_refused, (hipStream_t)hip_stream);
  if (rc != HSRANS_OK)
    return rc;
  // (the set's own word: the planes cut has passed every row the set sees, so this should never fire; it is reported if it does)
  return pgs->set != nullptr ? hsrans_gather_set_refused(ctx, pgs->set, hip_stream) : HSRANS_OK;
}
catch (...)
{
  return HSRANS_E_HIP;
}
