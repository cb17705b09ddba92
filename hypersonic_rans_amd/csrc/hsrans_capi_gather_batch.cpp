// hsrans_decode_device_gather_batch (include/hsrans_hip.h): byte ranges of many streams, one launch per table layout — the gather set
// (device plans bound to their streams, one uploaded record per member), the host-side cut of the ranges into one kind's entries
// (hsrans_gather_batch_tasks, a pure function), the argument checks and the launches (k_gather_set, kernels_gather.h, through
// launch_gather_set in hsrans_kernels.hip).  The task lists go through the context's task buffer as hsrans_decode_device_gather's do
// (gather_region_*, hsrans_capi_gather.cpp); range rules, plan test, the member's GatherSource and the cut of a range are the single
// call's own functions (hsrans_kernels.h, hsrans_internal.h).
// hsrans_decode_device_gather_batch_indirect: the same for ranges that are in device memory — no cut, no task buffer and no lock here: the
// device checks, sorts and cuts (k_set_cut, then one k_set_ranges per kind that has members, through launch_gather_set_ranges), the caller
// brings the workspace, and what the device refuses lands in a status word of the set's own (hsrans_gather_set_refused).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"

static_assert(sizeof(GatherSetRange) == sizeof(hsrans_member_range) && sizeof(hsrans_member_range) == 32 && sizeof(hsrans_gather_batch_task) == 32 && sizeof(hsrans_gather_member) == 24 &&
                  sizeof(GatherSetTask) == sizeof(hsrans_gather_batch_task),
              "gather batch ABI layout");

// (kGatherKinds, hsrans_kernels.h: k_gather_set's instantiations — kind = decode-table layout (kMode*), 3..5 with one table per workgroup)
constexpr uint32_t kGatherSetMaxMembers = 65536;

struct hsrans_gather_set
{
  hsrans_ctx *ctx = nullptr;
  std::vector<hsrans_dplan *> plans;
  std::vector<hsrans_gather_member> members; // what the cut needs of each
  std::vector<uint64_t> segment;             // ... and the L of each member's single call (gather_segment_of)
  std::vector<uint64_t> out_lo, out_hi;
  GatherSetMember *d_members = nullptr;
  uint32_t kind_members[kGatherKinds] = {};
  uint32_t kind_table_bytes[kGatherKinds] = {}; // the largest table among the kind's members, a multiple of 16
  // hsrans_decode_device_gather_batch_indirect: a member's position is its place in kind-major order (members sorted by kind, then index)
  uint32_t *d_position = nullptr;               // [members] the position of member m
  uint32_t *d_refused = nullptr;                // the set's own status word (kStatusBadRange: k_set_cut refused a call); no member plan's word is involved
  uint32_t kind_first[kGatherKinds + 1] = {};   // the first position of each kind ([6] = members)
  uint64_t kind_min_segment[kGatherKinds] = {}; // the smallest segment among the kind's members that can be cut (0: none can)
  hsrans_gather_set_info_t last{};              // the last call's part of hsrans_gather_set_info (under ctx->lock)
};

// tasks[m] = the tasks of member m's ranges, each range cut at the absolute multiples of segment[m]; false: a range is refused (its member,
// its extent) or a member that has tasks cannot be cut (segment 0)
static bool count_tasks(const hsrans_gather_member *members, uint32_t n_members, const uint64_t *segment, const hsrans_member_range *ranges, uint32_t count, uint64_t *tasks)
{
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_member_range &g = ranges[r];
    if (g.member >= n_members || !gather_extent_ok(g.offset, g.length, members[g.member].decoded_len))
      return false;
    if (g.length == 0)
      continue;
    if (segment[g.member] == 0)
      return false;
    tasks[g.member] += gather_range_tasks(g.offset, g.length, segment[g.member]);
  }
  return true;
}

// hsrans_gather_batch_tasks' body for segment lengths segment[m] and the task counts count_tasks gave
static size_t cut_batch(const hsrans_gather_member *members, uint32_t n_members, const uint64_t *segment, const uint64_t *tasks, const hsrans_member_range *ranges, uint32_t count,
                        uint32_t kind, uint32_t waves, hsrans_gather_batch_task *out, size_t capacity)
{
  const bool shared = kind >= 3;
  // shared: where each member's run starts in the launch (its tasks, then its padding); the cursor moves as the run is written
  std::vector<uint64_t> at;
  uint64_t total = 0;
  if (shared)
  {
    at.resize(n_members);
    for (uint32_t m = 0; m < n_members; m++)
    {
      at[m] = total;
      if (members[m].kind == kind)
        total += (tasks[m] + waves - 1) / waves * waves;
    }
  }
  uint64_t n = 0;
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_member_range &g = ranges[r];
    if (members[g.member].kind != kind)
      continue;
    const int64_t delta = (int64_t)(g.dst_offset - g.offset); // (modulo 2^64: the device adds it back the same way)
    uint64_t &pos = shared ? at[g.member] : n;
    gather_cut_range(g.offset, g.length, segment[g.member], [&](uint64_t b, uint64_t e) {
      if (pos < capacity)
        out[pos] = hsrans_gather_batch_task{b, e, delta, g.member, 0};
      pos++;
    });
  }
  if (!shared)
    return (size_t)n;
  for (uint32_t m = 0; m < n_members; m++)
    if (members[m].kind == kind)
      for (const uint64_t end = at[m] + (waves - tasks[m] % waves) % waves; at[m] < end; at[m]++)
        if (at[m] < capacity)
          out[at[m]] = hsrans_gather_batch_task{0, 0, 0, m, 0};
  return (size_t)total;
}

// the set's status word, and the byte-plane gather objects' (hsrans_internal.h)
int refusal_word_create(hsrans_ctx *ctx, uint32_t **word)
{
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)word, sizeof(uint32_t)) != hipSuccess || hipMemset(*word, 0, sizeof(uint32_t)) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  return HSRANS_OK;
}

int refusal_word_take(uint32_t *word, hipStream_t s)
{
  uint32_t status = 0xFFFFFFFF;
  if (hipMemcpyAsync(&status, word, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  if (status == 0)
    return HSRANS_OK;
  if (hipMemsetAsync(word, 0, 4, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_E_DEVICE;
}

extern "C"
{

size_t hsrans_gather_batch_tasks(const hsrans_gather_member *members, uint32_t n_members, const hsrans_member_range *ranges, uint32_t count, uint32_t kind, uint32_t waves,
                                 hsrans_gather_batch_task *out, size_t capacity)
{
  if ((members == nullptr && n_members > 0) || (ranges == nullptr && count > 0) || (out == nullptr && capacity > 0) || kind >= kGatherKinds || waves == 0)
    return 0;
  try
  {
    std::vector<uint64_t> segment(n_members), tasks(n_members, 0);
    for (uint32_t m = 0; m < n_members; m++)
      segment[m] = hsrans_gather_segment(members[m].decoded_len, members[m].n_chains, members[m].states, members[m].interval);
    if (!count_tasks(members, n_members, segment.data(), ranges, count, tasks.data()))
      return 0;
    return cut_batch(members, n_members, segment.data(), tasks.data(), ranges, count, kind, waves, out, capacity);
  }
  catch (const std::bad_alloc &)
  {
    return 0;
  }
}

int hsrans_gather_set_create(hsrans_ctx *ctx, hsrans_dplan *const *dplans, const void *const *d_streams, const size_t *stream_lengths, uint32_t count, hsrans_gather_set **out_set)
{
  if (out_set != nullptr)
    *out_set = nullptr;
  if (ctx == nullptr || dplans == nullptr || d_streams == nullptr || stream_lengths == nullptr || out_set == nullptr || count == 0 || count > kGatherSetMaxMembers)
    return HSRANS_E_ARG;
  for (uint32_t k = 0; k < count; k++)
    if (dplans[k] == nullptr || dplans[k]->ctx != ctx || d_streams[k] == nullptr || ((uintptr_t)d_streams[k] & 15) != 0)
      return HSRANS_E_ARG;
  for (uint32_t k = 0; k < count; k++)
    if (!gather_plan_ok(dplans[k], stream_lengths[k]))
      return HSRANS_E_FORMAT;
  hsrans_gather_set *set = new (std::nothrow) hsrans_gather_set;
  if (set == nullptr)
    return HSRANS_E_HIP;
  std::vector<GatherSetMember> recs(count);
  set->ctx = ctx;
  set->plans.assign(dplans, dplans + count);
  set->members.resize(count);
  set->segment.resize(count);
  set->out_lo.resize(count);
  set->out_hi.resize(count);
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_dplan *d = dplans[k];
    const PlanHeader &h = d->hdr;
    // the member's kind: the table layout its single gather uses (gather_shape's decision, whatever the task count)
    const GatherShape shape = gather_shape(d->tuning, h, ctx->geom, gather_table_mode(d), 1);
    if (shape.mode < 0 || shape.mode >= (int)kGatherKinds || shape.shared != (shape.mode >= 3))
    {
      delete set;
      return HSRANS_E_FORMAT;
    }
    const uint32_t kind = (uint32_t)shape.mode;
    set->members[k] = hsrans_gather_member{h.decoded_len, h.n_chains, h.states, h.interval, kind};
    set->segment[k] = gather_segment_of(d);
    set->out_lo[k] = d->out_lo;
    set->out_hi[k] = d->out_hi;
    set->kind_members[kind]++;
    const uint32_t table_bytes = gather_table_bytes(shape.mode, h.bits);
    if (table_bytes > set->kind_table_bytes[kind])
      set->kind_table_bytes[kind] = table_bytes;
    GatherSetMember &rec = recs[k];
    rec.src = gather_source_of(d, d_streams[k], stream_lengths[k]);
    rec.segment = set->segment[k];
    rec.decoded_len = h.decoded_len;
    rec.out_lo = d->out_lo;
    rec.out_hi = d->out_hi;
    rec.states = h.states;
    rec.bits = h.bits;
    if (set->segment[k] != 0 && (set->kind_min_segment[kind] == 0 || set->segment[k] < set->kind_min_segment[kind]))
      set->kind_min_segment[kind] = set->segment[k];
  }
  // positions: kind-major, inside a kind by member index
  std::vector<uint32_t> position(count, 0);
  for (uint32_t kind = 0; kind < kGatherKinds; kind++)
    set->kind_first[kind + 1] = set->kind_first[kind] + set->kind_members[kind];
  {
    uint32_t next[kGatherKinds];
    for (uint32_t kind = 0; kind < kGatherKinds; kind++)
      next[kind] = set->kind_first[kind];
    for (uint32_t k = 0; k < count; k++)
      position[k] = next[set->members[k].kind]++;
  }
  // the records go up once, here (a synchronous copy: they are in place when the call returns)
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void **)&set->d_members, count * sizeof(GatherSetMember)) != hipSuccess ||
      hipMemcpy(set->d_members, recs.data(), count * sizeof(GatherSetMember), hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc((void **)&set->d_position, (size_t)count * sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(set->d_position, position.data(), (size_t)count * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
      refusal_word_create(ctx, &set->d_refused) != HSRANS_OK)
  {
    (void)hipGetLastError();
    hsrans_gather_set_destroy(set);
    return HSRANS_E_HIP;
  }
  set->last.members = count;
  *out_set = set;
  return HSRANS_OK;
}

void hsrans_gather_set_destroy(hsrans_gather_set *set)
{
  if (set == nullptr)
    return;
  if (set->d_members != nullptr)
    (void)hipFree(set->d_members);
  if (set->d_position != nullptr)
    (void)hipFree(set->d_position);
  if (set->d_refused != nullptr)
    (void)hipFree(set->d_refused);
  delete set;
}

int hsrans_decode_device_gather_batch(hsrans_ctx *ctx, hsrans_gather_set *set, const hsrans_member_range *ranges, uint32_t count, void *d_dst, size_t dst_capacity,
                                      void *hip_stream)
{
  if (ctx == nullptr || set == nullptr || d_dst == nullptr || set->ctx != ctx || (ranges == nullptr && count > 0))
    return HSRANS_E_ARG;
  const uint32_t n_members = (uint32_t)set->members.size();
  bool any = false;
  for (uint32_t r = 0; r < count; r++)
  {
    const hsrans_member_range &g = ranges[r];
    if (g.member >= n_members || g.reserved != 0)
      return HSRANS_E_ARG;
    if (!gather_range_ok(g.offset, g.length, g.dst_offset, set->members[g.member].decoded_len, set->out_lo[g.member], set->out_hi[g.member], dst_capacity))
      return HSRANS_E_ARG;
    any = any || g.length != 0;
  }
  std::lock_guard<std::mutex> lk(ctx->lock);
  hsrans_gather_set_info_t &last = set->last;
  last.launches = 0;
  for (uint32_t k = 0; k < kGatherKinds; k++)
    last.kind_tasks[k] = last.kind_entries[k] = last.kind_grid[k] = last.kind_waves[k] = last.kind_lds_bytes[k] = 0;
  if (!any)
    return HSRANS_OK;

  // per kind: its tasks, the launch shape they give (gather_shape's rule for the kind's largest table) and, with the waves per workgroup
  // known, the entries of its launch
  std::vector<uint64_t> tasks;
  try
  {
    tasks.assign(n_members, 0);
  }
  catch (const std::bad_alloc &)
  {
    return HSRANS_E_HIP;
  }
  if (!count_tasks(set->members.data(), n_members, set->segment.data(), ranges, count, tasks.data()))
    return HSRANS_E_ARG;
  uint64_t kind_tasks[kGatherKinds] = {}, kind_entries[kGatherKinds] = {}, all_entries = 0;
  GatherShape shapes[kGatherKinds] = {};
  size_t offset[kGatherKinds] = {};
  Carve lists;
  for (uint32_t m = 0; m < n_members; m++)
    kind_tasks[set->members[m].kind] += tasks[m];
  for (uint32_t k = 0; k < kGatherKinds; k++)
  {
    if (kind_tasks[k] == 0)
      continue;
    if (kind_tasks[k] > 0x7FFFFFFFu)
      return HSRANS_E_ARG;
    shapes[k] = gather_set_shape(ctx->geom, (int)k, k >= 3, set->kind_table_bytes[k], (uint32_t)kind_tasks[k]);
    const uint32_t waves = shapes[k].waves;
    if (k >= 3)
      for (uint32_t m = 0; m < n_members; m++)
        kind_entries[k] += set->members[m].kind == k ? (tasks[m] + waves - 1) / waves * waves : 0;
    else
      kind_entries[k] = kind_tasks[k];
    all_entries += kind_entries[k];
    if (all_entries > 0x7FFFFFFFu)
      return HSRANS_E_ARG;
    shapes[k].grid = (uint32_t)((kind_entries[k] + waves - 1) / waves);
    offset[k] = lists.take((size_t)kind_entries[k] * sizeof(GatherSetTask));
  }
  const size_t need = lists.close();
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;

  // all kinds' lists in one region of the context's task buffers: one stream-ordered copy in front of the launches
  // (not gather_region_upload: this call queues several launches and commits after a partial failure)
  GatherRegion region;
  const int rc = gather_region_take(ctx, need, &region);
  if (rc != HSRANS_OK)
    return rc;
  for (uint32_t k = 0; k < kGatherKinds; k++)
    if (kind_entries[k] != 0)
    {
      size_t n = 0;
      try
      {
        n = cut_batch(set->members.data(), n_members, set->segment.data(), tasks.data(), ranges, count, k, shapes[k].waves, (hsrans_gather_batch_task *)(region.host + offset[k]),
                      (size_t)kind_entries[k]);
      }
      catch (const std::bad_alloc &)
      {
        return HSRANS_E_HIP;
      }
      if (n != kind_entries[k])
        return HSRANS_E_ARG;
    }
  if (gather_region_order(ctx, s) != HSRANS_OK)
    return HSRANS_E_HIP;
  if (hipMemcpyAsync(region.dev, region.host, need, hipMemcpyHostToDevice, s) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  bool failed = false;
  for (uint32_t k = 0; k < kGatherKinds && !failed; k++)
  {
    if (kind_entries[k] == 0)
      continue;
    GatherSetParams sp{};
    sp.members = set->d_members;
    sp.tasks = (const GatherSetTask *)(region.dev + offset[k]);
    sp.n_tasks = (uint32_t)kind_entries[k];
    sp.dst = (uint8_t *)d_dst;
    sp.table_bytes = set->kind_table_bytes[k];
    failed = launch_gather_set(sp, shapes[k], s) != hipSuccess;
    if (failed)
      break;
    last.launches++;
    last.kind_tasks[k] = (uint32_t)kind_tasks[k];
    last.kind_entries[k] = (uint32_t)kind_entries[k];
    last.kind_grid[k] = shapes[k].grid;
    last.kind_waves[k] = shapes[k].waves;
    last.kind_lds_bytes[k] = shapes[k].lds;
  }
  if (failed)
    (void)hipGetLastError();
  // (the region is committed whenever anything that reads it was queued: a launch that did go out must not see its list overwritten)
  if (last.launches != 0 || !failed)
  {
    const int rc_commit = gather_region_commit(ctx, region, s);
    if (rc_commit != HSRANS_OK)
      return rc_commit;
  }
  return failed ? HSRANS_E_HIP : HSRANS_OK;
}

// the launches of an indirect call on the set: one shape per kind that has members (grid 0 elsewhere), from what the host knows
static void indirect_shapes(const hsrans_gather_set *set, uint32_t max_count, size_t dst_capacity, GatherShape shapes[kGatherKinds])
{
  for (uint32_t k = 0; k < kGatherKinds; k++)
  {
    shapes[k] = GatherShape{};
    if (set->kind_members[k] != 0)
      shapes[k] = gather_set_ranges_shape(set->ctx->geom, (int)k, k >= 3, set->kind_table_bytes[k], max_count, dst_capacity, set->kind_min_segment[k], set->kind_members[k]);
  }
}

size_t hsrans_gather_batch_workspace_bytes(uint32_t members, uint32_t max_count)
{
  if (members == 0 || members > kGatherSetMaxMembers)
    return 0;
  return (size_t)gather_set_ws(members, max_count).words * 4;
}

int hsrans_gather_set_indirect_info(const hsrans_gather_set *set, uint32_t max_count, size_t dst_capacity, hsrans_gather_set_info_t *info)
{
  if (set == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  *info = hsrans_gather_set_info_t{};
  info->members = (uint32_t)set->members.size();
  GatherShape shapes[kGatherKinds];
  indirect_shapes(set, max_count, dst_capacity, shapes);
  for (uint32_t k = 0; k < kGatherKinds; k++)
  {
    info->kind_members[k] = set->kind_members[k];
    if (set->kind_members[k] == 0 || max_count == 0)
      continue;
    info->launches++;
    info->kind_grid[k] = shapes[k].grid;
    info->kind_waves[k] = shapes[k].waves;
    info->kind_lds_bytes[k] = shapes[k].lds;
  }
  return HSRANS_OK;
}

int hsrans_decode_device_gather_batch_indirect(hsrans_ctx *ctx, hsrans_gather_set *set, const hsrans_member_range *d_ranges, const uint32_t *d_count, uint32_t max_count, void *d_dst,
                                               size_t dst_capacity, void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
  if (ctx == nullptr || set == nullptr || d_ranges == nullptr || d_dst == nullptr || d_workspace == nullptr || set->ctx != ctx)
    return HSRANS_E_ARG;
  const uint32_t n_members = (uint32_t)set->members.size();
  if (((uintptr_t)d_ranges & 7) != 0 || ((uintptr_t)d_count & 3) != 0 || ((uintptr_t)d_workspace & 255) != 0 ||
      workspace_bytes < hsrans_gather_batch_workspace_bytes(n_members, max_count))
    return HSRANS_E_ARG;
  if (max_count == 0)
    return HSRANS_OK;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;

  GatherShape shapes[kGatherKinds];
  indirect_shapes(set, max_count, dst_capacity, shapes);
  GatherSetCutParams cp{};
  cp.ranges = (const GatherSetRange *)d_ranges;
  cp.count = d_count;
  cp.max_count = max_count;
  cp.n_members = n_members;
  cp.members = set->d_members;
  cp.position = set->d_position;
  cp.dst_capacity = dst_capacity;
  cp.workspace = (uint32_t *)d_workspace;
  cp.status = set->d_refused;
  for (uint32_t k = 0; k <= kGatherKinds; k++)
    cp.kind_first[k] = set->kind_first[k];
  for (uint32_t k = 0; k < kGatherKinds; k++)
    cp.kind_waves[k] = shapes[k].waves;
  if (launch_gather_set_ranges(cp, (uint8_t *)d_dst, shapes, set->kind_table_bytes, (hipStream_t)hip_stream) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  return HSRANS_OK;
}

int hsrans_gather_set_refused(hsrans_ctx *ctx, hsrans_gather_set *set, void *hip_stream)
{
  if (ctx == nullptr || set == nullptr || set->ctx != ctx)
    return HSRANS_E_ARG;
  return refusal_word_take(set->d_refused, (hipStream_t)hip_stream);
}

int hsrans_gather_set_status(hsrans_ctx *ctx, hsrans_gather_set *set, void *hip_stream, int *member_status)
{
  if (ctx == nullptr || set == nullptr || set->ctx != ctx)
    return HSRANS_E_ARG;
  int worst = HSRANS_OK;
  std::map<const hsrans_dplan *, int> seen; // (a plan that is a member twice: hsrans_dplan_status clears the word it reports)
  for (size_t k = 0; k < set->plans.size(); k++)
  {
    auto it = seen.find(set->plans[k]);
    const int rc = it != seen.end() ? it->second : hsrans_dplan_status(ctx, set->plans[k], hip_stream); // (the first synchronises the stream; the others find it idle)
    if (it == seen.end())
      seen.emplace(set->plans[k], rc);
    if (member_status != nullptr)
      member_status[k] = rc;
    if (rc != HSRANS_OK && worst == HSRANS_OK)
      worst = rc;
  }
  return worst;
}

int hsrans_gather_set_info(const hsrans_gather_set *set, hsrans_gather_set_info_t *info)
{
  if (set == nullptr || info == nullptr)
    return HSRANS_E_ARG;
  std::lock_guard<std::mutex> lk(set->ctx->lock);
  *info = set->last;
  info->members = (uint32_t)set->members.size();
  for (uint32_t k = 0; k < kGatherKinds; k++)
    info->kind_members[k] = set->kind_members[k];
  return HSRANS_OK;
}

} // extern "C"
