// hsrans_capi_encode_batch.cpp — hsrans_encode_device_batch: many independent raw / mt_ streams encoded by one launch per kernel kind.
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h).  Every member is what its single call (hsrans_encode_device_raw,
// hsrans_encode_device in hsrans_capi_encode.cpp) would make: the same checks, the same EncParams, the same per-wave code
// (hsrans_encode.hip encode_body and the bodies of the single calls' kernels); only where the parameters live changes — one record
// per member in device memory, and a task list that maps each workgroup to its member and block.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <iterator>
#include <mutex>
#include <utility>
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

// what the host knows of a member before launch (the single calls' own derivations)
struct Member
{
  bool raw = false;
  uint32_t S = 0;
  uint64_t slot_bytes = 0; // per block (raw: the one slot)
  uint32_t n_blocks = 1;
  uint32_t interval = 0;   // EncParams::interval
  uint32_t max_ck = 0;     // EncParams::max_ck
  size_t ck_slots = 1;
  // raw
  bool want_plan = false, listed = false;
  size_t n_ck = 0;
  uint32_t parts = 0;
  // carving
  size_t scratch_at = 0, ck_at = 0, header_at = 0, given_at = 0, groups_at = 0, meta_at = 0;
};

// the single calls' argument rules (hsrans_encode_device_raw, hsrans_encode_device), plus the batch's own: fields of the other container unset
bool check_member(const hsrans_encode_member &m, bool want_dplan, Member *out)
{
  Member r;
  if (!valid_codec(m.container, m.states, m.bits) || m.d_in == nullptr || m.d_out == nullptr || m.length == 0 || m.index_interval % 4 != 0 ||
      ((uintptr_t)m.d_in & 15) != 0 || ((uintptr_t)m.d_out & 15) != 0 || m.out_capacity < capacity(m.container, m.states, m.length) ||
      (uintptr_t)m.d_in + m.length < (uintptr_t)m.d_in || (uintptr_t)m.d_out + m.out_capacity < (uintptr_t)m.d_out)
    return false;
  r.S = (uint32_t)m.states;
  if (m.container == HSRANS_RAW)
  {
    if (m.block_size != 0 || m.length > 0x7FFF0000ull)
      return false;
    r.raw = true;
    r.listed = m.index_groups != nullptr && m.n_index_groups != 0;
    if (r.listed)
    {
      if (m.n_index_groups > 0x7FFFFFFFull)
        return false;
      for (size_t k = 0; k < m.n_index_groups; k++)
        if (m.index_groups[k] == 0 || (m.index_groups[k] % 4) != 0 || (k > 0 && m.index_groups[k] <= m.index_groups[k - 1]))
          return false;
    }
    if (m.hist != nullptr)
    {
      uint32_t sum = 0;
      for (int k = 0; k < 256; k++)
        sum += m.hist->symbolCount[k];
      if (sum != (1u << m.bits))
        return false;
    }
    r.want_plan = want_dplan && (r.listed || m.index_interval != 0);
    const uint64_t whole_groups = m.length / r.S;
    if (r.want_plan && r.listed)
      while (r.n_ck < m.n_index_groups && m.index_groups[r.n_ck] < whole_groups)
        r.n_ck++;
    else if (r.want_plan)
      r.n_ck = whole_groups >= 1 ? (size_t)((whole_groups - 1) / m.index_interval) : 0;
    r.slot_bytes = encode_slot_bytes(m.length, r.S);
    r.interval = r.want_plan && !r.listed ? m.index_interval : 0;
    r.max_ck = (uint32_t)r.n_ck;
    r.ck_slots = r.n_ck ? r.n_ck : 1;
    r.parts = (uint32_t)std::min<uint64_t>((m.length + kRawPartBytes - 1) / kRawPartBytes, kRawMaxParts);
  }
  else if (m.container == HSRANS_MT)
  {
    if (m.block_size == 0 || m.block_size % 64 != 0 || m.block_size > (1u << 30) || m.hist != nullptr || m.index_groups != nullptr || m.n_index_groups != 0)
      return false;
    r.n_blocks = encode_block_count(m.length, m.block_size, r.S);
    if (r.n_blocks == 0)
      return false;
    r.slot_bytes = encode_slot_bytes(m.block_size, r.S);
    r.interval = want_dplan ? m.index_interval : 0; // checkpoints only serve the plan
    r.max_ck = r.interval ? (m.block_size / r.S - 1) / r.interval : 0;
    r.ck_slots = (size_t)r.n_blocks * (r.max_ck ? r.max_ck : 1);
  }
  else
    return false;
  *out = r;
  return true;
}

// no two outputs overlap, no output overlaps an input
bool ranges_disjoint(const hsrans_encode_member *members, uint32_t count)
{
  std::vector<std::pair<uintptr_t, uintptr_t>> outs(count);
  for (uint32_t k = 0; k < count; k++)
    outs[k] = {(uintptr_t)members[k].d_out, (uintptr_t)members[k].d_out + members[k].out_capacity};
  std::sort(outs.begin(), outs.end());
  for (uint32_t k = 1; k < count; k++)
    if (outs[k].first < outs[k - 1].second)
      return false;
  for (uint32_t k = 0; k < count; k++) // the outputs are disjoint and sorted, so their ends are too: the last one starting below the input's end decides
  {
    const uintptr_t lo = (uintptr_t)members[k].d_in, hi = lo + members[k].length;
    auto it = std::lower_bound(outs.begin(), outs.end(), std::make_pair(hi, (uintptr_t)0));
    if (it != outs.begin() && std::prev(it)->second > lo)
      return false;
  }
  return true;
}

size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
} // namespace

extern "C" int hsrans_encode_device_batch(hsrans_ctx *ctx, hsrans_encode_member *members, uint32_t count, void *hip_stream, hsrans_dplan **out_dplans,
                                          hsrans_encode_batch_stats *stats)
{
  if (stats)
    *stats = hsrans_encode_batch_stats{};
  if (members == nullptr || count == 0 || count > kMaxMembers)
    return HSRANS_E_ARG;
  for (uint32_t k = 0; k < count; k++)
  {
    members[k].stream_length = 0;
    if (out_dplans)
      out_dplans[k] = nullptr;
  }
  if (ctx == nullptr)
    return HSRANS_E_ARG;

  // ---- every member checked before anything is launched ----
  std::vector<Member> mm(count);
  for (uint32_t k = 0; k < count; k++)
    if (!check_member(members[k], out_dplans != nullptr, &mm[k]))
      return HSRANS_E_ARG;
  if (!ranges_disjoint(members, count))
    return HSRANS_E_ARG;
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
  size_t scratch_bytes = 0, ck_bytes = 0, meta = 0;
  auto take = [](size_t *at, size_t bytes, size_t align) {
    *at = up(*at, align);
    const size_t here = *at;
    *at += bytes;
    return here;
  };
  for (uint32_t k = 0; k < count; k++)
  {
    mm[k].scratch_at = take(&scratch_bytes, (size_t)mm[k].n_blocks * mm[k].slot_bytes, 512);
    if (mm[k].raw)
      mm[k].ck_at = take(&ck_bytes, mm[k].ck_slots * ((size_t)mm[k].S * 4 + 4), 256);
  }
  bool any_raw_plan = false;
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && mm[k].want_plan)
    {
      mm[k].header_at = take(&ck_bytes, 16 + 512 + 4 * (size_t)mm[k].S, 16);
      any_raw_plan = true;
    }
  const size_t raw_down_bytes = ck_bytes; // the raw members' checkpoints and headers: one copy to the host
  for (uint32_t k = 0; k < count; k++)
    if (!mm[k].raw)
      mm[k].ck_at = take(&ck_bytes, mm[k].ck_slots * ((size_t)mm[k].S * 4 + 4), 256);

  const size_t off_params = take(&meta, (size_t)count * sizeof(EncParams), 256);
  const size_t off_raw_list = take(&meta, raw_list.size() * 4, 256);
  const size_t off_raw_parts = take(&meta, raw_parts.size() * sizeof(EncTask), 256);
  const size_t off_mt_tasks = take(&meta, mt_tasks.size() * sizeof(EncTask), 256);
  const size_t off_scan = take(&meta, scan_list.size() * 4, 256);
  const size_t off_headers = take(&meta, (size_t)count * sizeof(uint8_t *), 256);
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && members[k].hist != nullptr)
      mm[k].given_at = take(&meta, 512, 16);
  for (uint32_t k = 0; k < count; k++)
    if (mm[k].raw && mm[k].want_plan && mm[k].listed && mm[k].n_ck)
      mm[k].groups_at = take(&meta, mm[k].n_ck * 4, 16);
  const size_t upload_bytes = meta;
  const size_t off_results = take(&meta, (size_t)count * kEncResultWords * 8, 256);
  const size_t off_raw_counts = take(&meta, (size_t)n_raw * 1024, 16);
  const size_t zero_bytes = meta - off_results;
  for (uint32_t k = 0; k < count; k++)
  {
    const size_t nb = mm[k].n_blocks;
    // mt_: image_bytes, image_off [nb] u64, chain_count, chain_off [nb] u32, fits (16-byte aligned, 16 bytes), block counts [nb][256] u32
    mm[k].meta_at = take(&meta, mm[k].raw ? 16 : nb * 24 + 32 + nb * 1024, 256);
  }

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  if (!grow(&ctx->d_enc_scratch, &ctx->d_enc_scratch_cap, scratch_bytes) || !grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, meta) ||
      !grow(&ctx->d_enc_ck, &ctx->d_enc_ck_cap, std::max<size_t>(ck_bytes, 256)))
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
    EncParams ep{};
    ep.S = m.S;
    ep.bits = a.bits;
    ep.in = (const uint8_t *)a.d_in;
    ep.n = a.length;
    ep.out = (uint8_t *)a.d_out;
    ep.out_cap = a.out_capacity;
    ep.scratch = ctx->d_enc_scratch + m.scratch_at;
    ep.slot_bytes = m.slot_bytes;
    ep.n_blocks = m.n_blocks;
    ep.interval = m.interval;
    ep.max_ck = m.max_ck;
    ep.result = (uint64_t *)(d_meta + off_results) + (size_t)k * kEncResultWords;
    ep.ck_states = (uint32_t *)(ctx->d_enc_ck + m.ck_at);
    ep.ck_pos = ep.ck_states + m.ck_slots * m.S;
    uint8_t *own = d_meta + m.meta_at;
    headers[k] = nullptr;
    if (m.raw)
    {
      ep.block = a.length;
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
    {
      const size_t nb = m.n_blocks;
      ep.block = a.block_size;
      ep.image_bytes = (uint64_t *)own;
      ep.image_off = ep.image_bytes + nb;
      ep.chain_count = (uint32_t *)(ep.image_off + nb);
      ep.chain_off = ep.chain_count + nb;
      ep.fits = (uint64_t *)up((uintptr_t)(ep.chain_off + nb), 16);
      ep.raw_counts = (const uint32_t *)(ep.fits + 2);
    }
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
            launch_encode_batch(bt, s, &ctx->enc_batch_prepared, &launches) == hipSuccess &&
            hipMemcpyAsync(results.data(), d_meta + off_results, results.size() * 8, hipMemcpyDeviceToHost, s) == hipSuccess &&
            (!any_raw_plan || hipMemcpyAsync(raw_down.data(), ctx->d_enc_ck, raw_down_bytes, hipMemcpyDeviceToHost, s) == hipSuccess);
  if (hipStreamSynchronize(s) != hipSuccess || !ok) // (upload may be read until here)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  if (stats)
    stats->launches = launches;

  // ---- results; a raw member whose caller histogram misses a byte is the one failure on the device ----
  int rc = HSRANS_OK;
  std::vector<uint8_t> fine(count, 0);
  for (uint32_t k = 0; k < count; k++)
  {
    const uint64_t *r = &results[(size_t)k * kEncResultWords];
    fine[k] = r[1] == 1 && (!mm[k].raw || r[2] == 0);
    if (fine[k])
      members[k].stream_length = (size_t)r[0];
    else
      rc = HSRANS_E_DEVICE;
  }
  if (out_dplans == nullptr)
    return rc;

  auto fail_member = [&](uint32_t k) {
    members[k].stream_length = 0;
    if (out_dplans[k] != nullptr)
      hsrans_dplan_destroy(out_dplans[k]);
    out_dplans[k] = nullptr;
    if (rc == HSRANS_OK)
      rc = HSRANS_E_HIP;
  };

  // ---- raw plans: assembled on the host from the headers and checkpoints that came down (raw_plan_from_checkpoints, as the single call) ----
  std::vector<uint8_t> blob;
  std::vector<uint64_t> ck_group, ck_wfe;
  for (uint32_t k : raw_list)
  {
    const Member &m = mm[k];
    if (!fine[k] || !m.want_plan)
      continue;
    const hsrans_encode_member &a = members[k];
    const uint8_t *header = raw_down.data() + m.header_at;
    const uint32_t *ck_states = (const uint32_t *)(raw_down.data() + m.ck_at);
    const uint32_t *ck_pos = ck_states + m.ck_slots * m.S;
    ck_group.resize(m.n_ck);
    ck_wfe.resize(m.n_ck);
    for (size_t i = 0; i < m.n_ck; i++)
    {
      ck_group[i] = m.listed ? a.index_groups[i] : (uint64_t)(i + 1) * a.index_interval;
      ck_wfe[i] = ck_pos[i];
    }
    blob.resize(plan_capacity_chains(HSRANS_RAW, a.states, a.length, m.n_ck, 0));
    const size_t psize = raw_plan_from_checkpoints(a.states, a.bits, a.length, members[k].stream_length, (const uint16_t *)(header + 16),
                                                   (const uint32_t *)(header + 16 + 512), m.n_ck, ck_group.data(), ck_wfe.data(), ck_states,
                                                   m.listed ? 0 : a.index_interval, blob.data(), blob.size());
    if (psize == 0 || hsrans_dplan_create(ctx, blob.data(), psize, &out_dplans[k]) != HSRANS_OK)
      fail_member(k);
  }

  // ---- mt_ plans: written on the device by one K_plan launch over every block of the members, once their chain counts are known ----
  if (n_mt_members == 0)
    return rc;
  std::vector<PlanHeader> heads(count);
  std::vector<uint8_t> grouped(count, 0);
  bool any_plan = false;
  for (uint32_t k = 0; k < count; k++)
  {
    const Member &m = mm[k];
    if (m.raw || !fine[k])
      continue;
    const uint64_t *r = &results[(size_t)k * kEncResultWords];
    EncParams &ep = params[k];
    hsrans_dplan *d = r[2] == 0 || r[2] > 0xFFFFFFFFull ? nullptr : dplan_new(ctx);
    if (d == nullptr)
    {
      fail_member(k);
      continue;
    }
    PlanHeader &h = heads[k];
    h = mt_plan_header(m.S, members[k].bits, members[k].length, members[k].stream_length, (uint32_t)r[2]);
    h.shared_hist = r[3] == 1 ? 1 : 0; // exactly one block with a histogram (hsrans_host.cpp PlanBuilder::serialize)
    h.aux_off = h.shared_hist ? r[4] : 0;
    h.interval = ep.interval;
    grouped[k] = ep.interval != 0 && ep.n_blocks < h.n_chains;
    ep.group_split = grouped[k] ? group_parts_of(ep.max_ck + 1, std::min(group_parts_max(ctx->geom, ep.n_blocks), 64u)) : 1;
    DplanRegions reg;
    reg.counters = grouped[k];
    reg.plan = (size_t)plan_size(h.n_chains, h.n_pieces, h.states, 0);
    reg.groups = grouped[k] ? (size_t)ep.n_blocks * ep.group_split * sizeof(Group) : 0;
    reg.zero = kZeroThroughPlan;
    out_dplans[k] = d;
    if (dplan_arena(d, reg, s) != HSRANS_OK || hipMemcpyAsync(d->d_plan, &h, sizeof(h), hipMemcpyHostToDevice, s) != hipSuccess)
    {
      fail_member(k);
      continue;
    }
    ep.plan = d->d_plan;
    ep.groups = d->d_groups;
    ep.n_chains = h.n_chains;
    any_plan = true;
  }
  for (uint32_t k = 0; k < count; k++) // (members without a plan: their blocks return at once)
    if (!mm[k].raw && out_dplans[k] == nullptr)
      params[k].plan = nullptr;
  ok = !any_plan || (hipMemcpyAsync(d_meta + off_params, params, (size_t)count * sizeof(EncParams), hipMemcpyHostToDevice, s) == hipSuccess &&
                     launch_encode_plan_batch(bt.params, bt.mt_blocks, (uint32_t)mt_tasks.size(), s, &launches) == hipSuccess);
  if (hipStreamSynchronize(s) != hipSuccess || !ok) // (heads / params may be read until here)
  {
    (void)hipGetLastError();
    for (uint32_t k = 0; k < count; k++)
      if (!mm[k].raw && out_dplans[k] != nullptr)
        fail_member(k);
    return rc == HSRANS_OK || rc == HSRANS_E_DEVICE ? HSRANS_E_HIP : rc;
  }
  if (stats)
    stats->launches = launches;
  for (uint32_t k = 0; k < count; k++)
    if (!mm[k].raw && out_dplans[k] != nullptr)
      dplan_adopt(out_dplans[k], heads[k], grouped[k] ? params[k].n_blocks * params[k].group_split : 0, params[k].max_ck + 1, s);
  return rc;
}
