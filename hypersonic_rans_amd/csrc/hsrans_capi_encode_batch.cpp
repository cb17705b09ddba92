// hsrans_capi_encode_batch.cpp — hsrans_encode_device_batch: many independent raw / mt_ streams encoded by one launch per kernel kind.
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h).  Every member is what its single call (hsrans_encode_device_raw,
// hsrans_encode_device in hsrans_capi_encode.cpp) would make, through the same code: the same rules and shape (raw_shape, mt_shape), the
// same per-block arrays (mt_block_arrays), the same plan assembly (raw_plan; mt_plan_begin / mt_plan_adopt around K_plan) and the same
// per-wave code (hsrans_encode.hip encode_body and the bodies of the single calls' kernels); only where the parameters live changes —
// one record per member in device memory, and a task list that maps each workgroup to its member and block.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_encode.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"

namespace
{
constexpr uint32_t kMaxMembers = 65536;
constexpr uint64_t kRawPartBytes = 1 << 16; // input bytes per workgroup of the raw histogram / copy (launch_encode_raw's K_hist)
constexpr uint32_t kRawMaxParts = 4096;
constexpr size_t kMaxTasks = (size_t)1 << 24; // mt_ blocks of all members, and raw histogram / copy workgroups

// what the host knows of a member before launch: its single call's shape, and where the batch puts its parts
struct Member : EncShape
{
  bool raw = false;
  uint32_t parts = 0; // raw: histogram / copy workgroups
  size_t scratch_at = 0, ck_at = 0, header_at = 0, given_at = 0, groups_at = 0, meta_at = 0;
};

// the single calls' argument rules (raw_shape, mt_shape), plus the batch's own: fields of the other container unset, no range that wraps
bool check_member(const hsrans_encode_member &m, bool want_dplan, Member *out)
{
  if (!device_io_ok(m.d_in, m.d_out) || (uintptr_t)m.d_in + m.length < (uintptr_t)m.d_in || (uintptr_t)m.d_out + m.out_capacity < (uintptr_t)m.d_out)
    return false;
  out->raw = m.container == HSRANS_RAW;
  if (!out->raw)
    return m.container == HSRANS_MT && m.hist == nullptr && m.index_groups == nullptr && m.n_index_groups == 0 &&
           mt_shape(m.states, m.bits, m.length, m.out_capacity, m.block_size, m.index_interval, want_dplan, out);
  if (m.block_size != 0 || !raw_shape(m.states, m.bits, m.length, m.out_capacity, m.hist, m.index_interval, m.index_groups, m.n_index_groups, want_dplan, out))
    return false;
  out->parts = (uint32_t)std::min<uint64_t>((m.length + kRawPartBytes - 1) / kRawPartBytes, kRawMaxParts);
  return true;
}

// a member that ends without a stream: no length and no plan (one already made for it is destroyed)
void fail_member(hsrans_encode_member *members, hsrans_dplan **out_dplans, uint32_t k)
{
  members[k].stream_length = 0;
  if (out_dplans != nullptr && out_dplans[k] != nullptr)
  {
    hsrans_dplan_destroy(out_dplans[k]);
    out_dplans[k] = nullptr;
  }
}
} // namespace

extern "C" int hsrans_encode_device_batch(hsrans_ctx *ctx, hsrans_encode_member *members, uint32_t count, void *hip_stream, hsrans_dplan **out_dplans,
                                          hsrans_encode_batch_stats *stats)
try
{
  if (stats)
    *stats = hsrans_encode_batch_stats{};
  if (members == nullptr || count == 0 || count > kMaxMembers)
    return HSRANS_E_ARG;
  for (uint32_t k = 0; k < count; k++)
  {
    if (out_dplans)
      out_dplans[k] = nullptr; // (the caller's array may hold anything: nothing to destroy yet)
    fail_member(members, out_dplans, k);
  }
  if (ctx == nullptr)
    return HSRANS_E_ARG;

  // ---- every member checked before anything is launched ----
  std::vector<Member> mm(count);
  for (uint32_t k = 0; k < count; k++)
    if (!check_member(members[k], out_dplans != nullptr, &mm[k]))
      return HSRANS_E_ARG;
  {
    std::vector<Span> spans; // (raw_shape / mt_shape refuse an empty input and a capacity below hsrans_capacity: no span here is empty)
    spans.reserve(2 * (size_t)count);
    for (uint32_t k = 0; k < count; k++)
    {
      spans.push_back({(uintptr_t)members[k].d_out, (uintptr_t)members[k].d_out + members[k].out_capacity, true});
      spans.push_back({(uintptr_t)members[k].d_in, (uintptr_t)members[k].d_in + members[k].length, false});
    }
    if (!spans_disjoint(spans))
      return HSRANS_E_ARG;
  }
  size_t n_tasks[2] = {0, 0}; // raw histogram / copy workgroups, mt_ blocks (workgroups of 256 threads in one grid: fewer than 2^24)
  for (uint32_t k = 0; k < count; k++)
    n_tasks[mm[k].raw ? 0 : 1] += mm[k].raw ? mm[k].parts : mm[k].n_blocks;
  if (n_tasks[0] >= kMaxTasks || n_tasks[1] >= kMaxTasks)
    return HSRANS_E_ARG;

  // ---- task lists: raw coding wavefronts and mt_ blocks, 64-state members first (one launch per state count) ----
  std::vector<uint32_t> raw_list, scan_list;
  std::vector<EncTask> raw_parts, mt_tasks;
  uint32_t n_raw64 = 0, n_mt64 = 0, n_mt_members = 0;
  for (uint32_t S : {64u, 32u})
    for (uint32_t k = 0; k < count; k++)
    {
      const Member &m = mm[k];
      if (m.S != S)
        continue;
      if (m.raw)
      {
        raw_list.push_back(k);
        n_raw64 += S == 64;
        for (uint32_t p = 0; p < m.parts; p++)
          raw_parts.push_back(EncTask{k, p, m.parts});
      }
      else
      {
        n_mt_members++;
        for (uint32_t b = 0; b < m.n_blocks; b++)
          mt_tasks.push_back(EncTask{k, b, 0});
        n_mt64 += S == 64 ? m.n_blocks : 0;
        if (m.n_blocks > kEncSelfScanBlocks)
          scan_list.push_back(k);
      }
    }
  const uint32_t n_raw = (uint32_t)raw_list.size();
  if (stats)
  {
    stats->raw_members = n_raw;
    stats->mt_members = n_mt_members;
    stats->mt_blocks = (uint32_t)mt_tasks.size();
  }

  // ---- carving: the context's scratch (slots), checkpoint (raw members', their headers, then mt_ members') and meta buffers ----
  // meta: [upload: params | raw list | raw parts | mt_ tasks | scan list | header pointers | hists | group lists]
  //       [zeroed: result words (8 per member) | raw counts (256 per raw member)] [per member: image sizes / offsets, chain counts, block counts]
  Carve scratch, ck, meta;
  for (uint32_t k = 0; k < count; k++)
  {
    mm[k].scratch_at = scratch.take((size_t)mm[k].n_blocks * mm[k].slot_bytes, 512);
    if (mm[k].raw)
      mm[k].ck_at = ck.take(ck_region_bytes(mm[k].ck_slots, mm[k].S), 256);
  }
  bool any_raw_plan = false;
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && mm[k].want_plan)
    {
      mm[k].header_at = ck.take(16 + 512 + 4 * (size_t)mm[k].S, 16);
      any_raw_plan = true;
    }
  const size_t raw_down_bytes = ck.at; // the raw members' checkpoints and headers: one copy to the host
  for (uint32_t k = 0; k < count; k++)
    if (!mm[k].raw)
      mm[k].ck_at = ck.take(ck_region_bytes(mm[k].ck_slots, mm[k].S), 256);

  const size_t off_params = meta.take((size_t)count * sizeof(EncParams), 256);
  const size_t off_raw_list = meta.take(raw_list.size() * 4, 256);
  const size_t off_raw_parts = meta.take(raw_parts.size() * sizeof(EncTask), 256);
  const size_t off_mt_tasks = meta.take(mt_tasks.size() * sizeof(EncTask), 256);
  const size_t off_scan = meta.take(scan_list.size() * 4, 256);
  const size_t off_headers = meta.take((size_t)count * sizeof(uint8_t *), 256);
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && members[k].hist != nullptr)
      mm[k].given_at = meta.take(512, 16);
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && mm[k].want_plan && mm[k].listed && mm[k].n_ck)
      mm[k].groups_at = meta.take(mm[k].n_ck * 4, 16);
  const size_t upload_bytes = meta.at;
  const size_t off_results = meta.take((size_t)count * kEncResultWords * 8, 256);
  const size_t off_raw_counts = meta.take((size_t)n_raw * 1024, 16);
  const size_t zero_bytes = meta.at - off_results;
  for (uint32_t k = 0; k < count; k++) // (raw: image_bytes, image_off)
    mm[k].meta_at = meta.take(mm[k].raw ? 16 : mt_block_arrays_bytes(mm[k].n_blocks), 256);

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return HSRANS_E_HIP;
  if (!encoder_buffers(ctx, scratch.at, meta.at, std::max<size_t>(ck.at, 256)))
    return HSRANS_E_HIP;
  uint8_t *const d_meta = ctx->d_enc_meta;

  // ---- the members' EncParams, as the single calls fill them ----
  std::vector<uint8_t> upload(upload_bytes);
  EncParams *params = (EncParams *)(upload.data() + off_params);
  uint8_t **headers = (uint8_t **)(upload.data() + off_headers);
  uint32_t raw_index = 0;
  std::vector<uint32_t> raw_slot(count, 0); // a raw member's place among the raw counts
  for (uint32_t k : raw_list)
    raw_slot[k] = raw_index++;
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_encode_member &a = members[k];
    const Member &m = mm[k];
    EncParams ep = m.params(a.d_in, a.d_out, a.out_capacity);
    ep.scratch = ctx->d_enc_scratch + m.scratch_at;
    ep.result = (uint64_t *)(d_meta + off_results) + (size_t)k * kEncResultWords;
    ck_region(&ep, ctx->d_enc_ck + m.ck_at, m.ck_slots, m.S);
    uint8_t *own = d_meta + m.meta_at;
    headers[k] = nullptr;
    if (m.raw)
    {
      ep.image_bytes = (uint64_t *)own;
      ep.image_off = ep.image_bytes + 1;
      ep.raw_counts = (const uint32_t *)(d_meta + off_raw_counts) + (size_t)raw_slot[k] * 256;
      if (a.hist != nullptr)
      {
        memcpy(upload.data() + m.given_at, a.hist->symbolCount, 512);
        ep.given_counts = (const uint16_t *)(d_meta + m.given_at);
      }
      if (m.want_plan && m.listed && m.n_ck)
      {
        uint32_t *g = (uint32_t *)(upload.data() + m.groups_at);
        for (size_t i = 0; i < m.n_ck; i++)
          g[i] = (uint32_t)a.index_groups[i];
        ep.ck_groups = (const uint32_t *)(d_meta + m.groups_at);
        ep.n_ck_groups = (uint32_t)m.n_ck;
      }
      if (m.want_plan)
        headers[k] = ctx->d_enc_ck + m.header_at;
    }
    else
      mt_block_arrays(&ep, own);
    params[k] = ep;
  }
  memcpy(upload.data() + off_raw_list, raw_list.data(), raw_list.size() * 4);
  memcpy(upload.data() + off_raw_parts, raw_parts.data(), raw_parts.size() * sizeof(EncTask));
  memcpy(upload.data() + off_mt_tasks, mt_tasks.data(), mt_tasks.size() * sizeof(EncTask));
  memcpy(upload.data() + off_scan, scan_list.data(), scan_list.size() * 4);

  EncBatch bt{};
  bt.params = (const EncParams *)(d_meta + off_params);
  bt.raw_parts = (const EncTask *)(d_meta + off_raw_parts);
  bt.n_raw_parts = (uint32_t)raw_parts.size();
  bt.raw_members = (const uint32_t *)(d_meta + off_raw_list);
  bt.n_raw64 = n_raw64;
  bt.n_raw32 = n_raw - n_raw64;
  bt.raw_headers = (uint8_t *const *)(d_meta + off_headers);
  bt.mt_blocks = (const EncTask *)(d_meta + off_mt_tasks);
  bt.n_mt64_blocks = n_mt64;
  bt.n_mt32_blocks = (uint32_t)mt_tasks.size() - n_mt64;
  bt.scan_members = (const uint32_t *)(d_meta + off_scan);
  bt.n_scan = (uint32_t)scan_list.size();
  bt.zero = d_meta + off_results;
  bt.zero_bytes = zero_bytes;

  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t launches = 0;
  std::vector<uint64_t> results((size_t)count * kEncResultWords);
  std::vector<uint8_t> raw_down(any_raw_plan ? raw_down_bytes : 0);
  bool ok = hipMemcpyAsync(d_meta, upload.data(), upload_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
            launch_encode_batch(bt, ctx->geom.num_cus, s, &launches) == hipSuccess &&
            hipMemcpyAsync(results.data(), d_meta + off_results, results.size() * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
            (!any_raw_plan || hipMemcpyAsync(raw_down.data(), ctx->d_enc_ck, raw_down_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
  if (!stream_settle(s, ok)) // (upload may be read until here)
    return HSRANS_E_HIP;
  if (stats)
    stats->launches = launches;

  // ---- results; a raw member whose caller histogram misses a byte is the one failure on the device ----
  int rc = HSRANS_OK;
  std::vector<uint8_t> fine(count, 0);
  for (uint32_t k = 0; k < count; k++)
  {
    const uint64_t *r = &results[(size_t)k * kEncResultWords];
    fine[k] = enc_result_ok(r, mm[k].raw); // (an mt_ member's word 2 is its chain count)
    if (fine[k])
      members[k].stream_length = (size_t)r[0];
    else
      rc = HSRANS_E_DEVICE;
  }
  if (out_dplans == nullptr)
    return rc;

  // ---- raw plans: assembled on the host from the headers and checkpoints that came down, as the single call does (raw_plan) ----
  for (uint32_t k : raw_list)
  {
    const Member &m = mm[k];
    if (!fine[k] || !m.want_plan)
      continue;
    EncParams down{}; // (the member's checkpoint region in the host's copy)
    ck_region(&down, raw_down.data() + m.ck_at, m.ck_slots, m.S);
    if (raw_plan(ctx, m, members[k].stream_length, members[k].index_groups, raw_down.data() + m.header_at, down.ck_states, down.ck_pos, nullptr, 0, nullptr,
                 &out_dplans[k]) == 0)
    {
      fail_member(members, out_dplans, k);
      rc = rc == HSRANS_OK ? HSRANS_E_HIP : rc;
    }
  }

  // ---- mt_ plans: written on the device by one K_plan launch over every block of the members, once their chain counts are known ----
  if (n_mt_members == 0)
    return rc;
  std::vector<PlanHeader> heads(count);
  bool any_plan = false;
  for (uint32_t k = 0; k < count; k++) // (members without a plan keep EncParams::plan null: their blocks return at once)
  {
    if (mm[k].raw || !fine[k])
      continue;
    out_dplans[k] = mt_plan_begin(ctx, &params[k], &results[(size_t)k * kEncResultWords], &heads[k], s);
    if (out_dplans[k] == nullptr)
    {
      fail_member(members, out_dplans, k);
      rc = rc == HSRANS_OK ? HSRANS_E_HIP : rc;
    }
    any_plan = any_plan || out_dplans[k] != nullptr;
  }
  ok = !any_plan || (hipMemcpyAsync(d_meta + off_params, params, (size_t)count * sizeof(EncParams), hipMemcpyHostToDevice, s) == hipSuccess &&
                     launch_encode_plan_batch(bt.params, bt.mt_blocks, (uint32_t)mt_tasks.size(), s, &launches) == hipSuccess);
  if (!stream_settle(s, ok)) // (heads / params may be read until here)
  {
    for (uint32_t k = 0; k < count; k++)
      if (!mm[k].raw && out_dplans[k] != nullptr)
        fail_member(members, out_dplans, k);
    return HSRANS_E_HIP; // (whatever rc held: HSRANS_OK, or a member's HSRANS_E_DEVICE / HSRANS_E_HIP)
  }
  if (stats)
    stats->launches = launches;
  for (uint32_t k = 0; k < count; k++)
    if (!mm[k].raw && out_dplans[k] != nullptr)
      mt_plan_adopt(out_dplans[k], params[k], heads[k], s);
  return rc;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI; thrown only after the caller's arrays were reset)
{
  for (uint32_t k = 0; k < count; k++)
    fail_member(members, out_dplans, k);
  return HSRANS_E_HIP;
}
