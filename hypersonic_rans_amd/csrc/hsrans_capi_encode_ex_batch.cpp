// hsrans_capi_encode_ex_batch.cpp — hsrans_encode_device_ex_batch: many block_ / carried-state mt_ streams, one launch per kernel kind.
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h).  Every member is what hsrans_encode_device_ex's chain path
// (hsrans_capi_encode.cpp) would make, through the same code: the same rules (ex_route), the same summaries request (chain_units), the same
// host walk (chain_walk), the same chain preparation (chain_prepare, chain_params), the same plan finish (chain_plan_finish) and the same
// per-wave code (the bodies of enc_place.h); only where the parameters live changes — one record per member in device memory, and task
// lists that map each workgroup to its member and unit, block or part.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
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
constexpr size_t kMaxTasks = (size_t)1 << 24; // summary units of all members, and gather workgroups

// a member that ends without a stream: its code, no length, no plan size and no device plan (one already made for it is destroyed)
void member_fail(hsrans_encode_ex_member *members, hsrans_dplan **out_dplans, uint32_t k, int rc)
{
  members[k].stream_length = 0;
  members[k].rc = rc;
  if (members[k].opts)
    members[k].opts->plan_size = 0;
  if (out_dplans != nullptr && out_dplans[k] != nullptr)
  {
    hsrans_dplan_destroy(out_dplans[k]);
    out_dplans[k] = nullptr;
  }
}

int all_fail(hsrans_encode_ex_member *members, uint32_t count, hsrans_dplan **out_dplans, int rc)
{
  for (uint32_t k = 0; k < count; k++)
    member_fail(members, out_dplans, k, rc);
  return rc;
}

double us_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
  return std::chrono::duration<double, std::micro>(b - a).count();
}
} // namespace

extern "C" int hsrans_encode_device_ex_batch(hsrans_ctx *ctx, hsrans_encode_ex_member *members, uint32_t count, void *hip_stream, hsrans_dplan **out_dplans,
                                             hsrans_encode_ex_batch_stats *stats)
try
{
  if (stats)
    *stats = hsrans_encode_ex_batch_stats{};
  if (members == nullptr || count == 0 || count > kMaxMembers)
    return HSRANS_E_ARG;
  if (out_dplans)
    for (uint32_t k = 0; k < count; k++)
      out_dplans[k] = nullptr; // (the caller's array may hold anything: nothing to destroy yet)
  if (ctx == nullptr)
    return all_fail(members, count, out_dplans, HSRANS_E_ARG);

  // ---- every member checked before anything is launched: the single call's rules, then the batch's own ----
  std::vector<ChainJob> jobs(count);
  size_t n_unit_tasks = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_encode_ex_member &m = members[k];
    if ((uintptr_t)m.d_in + m.length < (uintptr_t)m.d_in || (uintptr_t)m.d_out + m.out_capacity < (uintptr_t)m.d_out ||
        ex_route(m.container, m.states, m.bits, m.d_in, m.length, m.d_out, m.out_capacity, m.opts, &jobs[k]) != kExChain || !chain_units(&jobs[k]))
      return all_fail(members, count, out_dplans, HSRANS_E_ARG);
    n_unit_tasks += jobs[k].n_units;
  }
  if (n_unit_tasks >= kMaxTasks)
    return all_fail(members, count, out_dplans, HSRANS_E_ARG);
  {
    // the batch's own rules: outputs and inputs by the overlap rule, and no two members share an opts object or a plan_out range
    // (ex_route refuses an empty input and a capacity below hsrans_capacity: no span here is empty)
    std::vector<Span> io, opts, plans;
    io.reserve(2 * (size_t)count);
    for (uint32_t k = 0; k < count; k++)
    {
      const hsrans_encode_ex_member &m = members[k];
      io.push_back({(uintptr_t)m.d_out, (uintptr_t)m.d_out + m.out_capacity, true});
      io.push_back({(uintptr_t)m.d_in, (uintptr_t)m.d_in + m.length, false});
      if (m.opts != nullptr)
        opts.push_back({(uintptr_t)m.opts, (uintptr_t)m.opts + sizeof(hsrans_encode_opts), true});
      if (jobs[k].want_plan)
        plans.push_back({(uintptr_t)m.opts->plan_out, (uintptr_t)m.opts->plan_out + std::max<size_t>(m.opts->plan_capacity, 1), true});
    }
    if (!spans_disjoint(io) || !spans_disjoint(opts) || !spans_disjoint(plans))
      return all_fail(members, count, out_dplans, HSRANS_E_ARG);
  }

  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t s = (hipStream_t)hip_stream;
  uint32_t launches = 0;
  if (stats)
    for (uint32_t k = 0; k < count; k++)
    {
      stats->block_members += jobs[k].container == HSRANS_BLOCK;
      stats->mt_members += jobs[k].container == HSRANS_MT;
      stats->units += (uint32_t)jobs[k].n_units;
    }

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (!encoder_ready(ctx))
    return all_fail(members, count, out_dplans, HSRANS_E_HIP);

  // ---- a. the unit summaries of all members: one launch over the (member, unit) tasks, one over the adaptive members' whole units ----
  // meta: [upload: params | unit tasks | cost tasks | summary pointers | table pointers | one logarithm table per width present] [summaries]
  Carve meta;
  size_t table_at[16] = {};
  std::vector<EncTask> unit_tasks, cost_tasks;
  unit_tasks.reserve(n_unit_tasks);
  for (uint32_t k = 0; k < count; k++)
    for (size_t u = 0; u < jobs[k].n_units; u++)
    {
      unit_tasks.push_back(EncTask{k, (uint32_t)u, 0});
      if (!jobs[k].fixed && (u + 1) * jobs[k].unit <= jobs[k].length) // (a short last unit is never a candidate: its cost stays 0)
        cost_tasks.push_back(EncTask{k, (uint32_t)u, 0});
    }
  const size_t off_params = meta.take((size_t)count * sizeof(EncParams), 256);
  const size_t off_unit_tasks = meta.take(unit_tasks.size() * sizeof(EncTask), 256);
  const size_t off_cost_tasks = meta.take(cost_tasks.size() * sizeof(EncTask), 256);
  const size_t off_sum_ptrs = meta.take((size_t)count * sizeof(void *), 256);
  const size_t off_table_ptrs = meta.take((size_t)count * sizeof(void *), 256);
  bool width_present[16] = {};
  for (uint32_t k = 0; k < count; k++)
    width_present[jobs[k].bits] = width_present[jobs[k].bits] || !jobs[k].fixed;
  for (uint32_t bits = 0; bits < 16; bits++)
    if (width_present[bits])
      table_at[bits] = meta.take((((size_t)1 << bits) + 1) * 4, 256);
  const size_t upload1_bytes = meta.at;
  const size_t off_summaries = meta.close();
  std::vector<size_t> sum_at(count);
  for (uint32_t k = 0; k < count; k++)
    sum_at[k] = meta.take(jobs[k].n_units * sizeof(UnitSummary), 256);
  const size_t summaries_bytes = meta.at - off_summaries;
  if (!grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, meta.at))
    return all_fail(members, count, out_dplans, HSRANS_E_HIP);
  uint8_t *d_meta = ctx->d_enc_meta;
  std::vector<uint8_t> upload(upload1_bytes), summaries(summaries_bytes);
  {
    EncParams *params = (EncParams *)(upload.data() + off_params);
    uint8_t **sum_ptrs = (uint8_t **)(upload.data() + off_sum_ptrs);
    const float **table_ptrs = (const float **)(upload.data() + off_table_ptrs);
    for (uint32_t k = 0; k < count; k++)
    {
      params[k] = chain_units_params(jobs[k]);
      sum_ptrs[k] = d_meta + sum_at[k];
      table_ptrs[k] = jobs[k].fixed ? nullptr : (const float *)(d_meta + table_at[jobs[k].bits]);
    }
    if (!unit_tasks.empty())
      memcpy(upload.data() + off_unit_tasks, unit_tasks.data(), unit_tasks.size() * sizeof(EncTask));
    if (!cost_tasks.empty())
      memcpy(upload.data() + off_cost_tasks, cost_tasks.data(), cost_tasks.size() * sizeof(EncTask));
    for (uint32_t bits = 0; bits < 16; bits++)
      if (width_present[bits])
        walk_log_table(bits, (float *)(upload.data() + table_at[bits]));
  }
  bool ok = hipMemcpyAsync(d_meta, upload.data(), upload1_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
            launch_unit_summaries_batch((const EncParams *)(d_meta + off_params), (const EncTask *)(d_meta + off_unit_tasks), (uint32_t)unit_tasks.size(),
                                        (const EncTask *)(d_meta + off_cost_tasks), (uint32_t)cost_tasks.size(), (uint8_t *const *)(d_meta + off_sum_ptrs),
                                        (const float *const *)(d_meta + off_table_ptrs), s, &launches) == hipSuccess &&
            hipMemcpyAsync(summaries.data(), d_meta + off_summaries, summaries_bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  if (!stream_settle(s, ok)) // (upload may be read until here)
    return all_fail(members, count, out_dplans, HSRANS_E_HIP);
  const auto t1 = std::chrono::steady_clock::now();

  // ---- b. the host walks, member by member, and what the chain needs of their blocks; a plan that does not fit leaves its member out ----
  int rc = HSRANS_OK;
  std::vector<uint32_t> coded; // the members of the coding launch
  for (uint32_t k = 0; k < count; k++)
  {
    members[k].stream_length = 0;
    members[k].rc = HSRANS_OK;
    if (!chain_walk(&jobs[k], (const UnitSummary *)(summaries.data() + (sum_at[k] - off_summaries))))
    {
      member_fail(members, out_dplans, k, HSRANS_E_DEVICE); // (the summaries are inconsistent: not what the device should have written)
      continue;
    }
    chain_prepare(&jobs[k]);
    if (jobs[k].want_plan && chain_plan_bytes(jobs[k]) > members[k].opts->plan_capacity)
    {
      member_fail(members, out_dplans, k, HSRANS_E_ARG);
      continue;
    }
    coded.push_back(k);
  }
  const auto t2 = std::chrono::steady_clock::now();

  // ---- c. the chains: a workgroup of one wavefront per member, the longest first, one launch per state count; then one gather ----
  // meta:  [upload: params | member list | gather tasks | per member: blocks, counts, listed checkpoints] [down: per member: image sizes, offsets, result]
  // ck:    [members with a plan: checkpoint states, positions, block states] [the others' one unused slot]
  std::stable_sort(coded.begin(), coded.end(), [&](uint32_t a, uint32_t b) {
    return jobs[a].S != jobs[b].S ? jobs[a].S > jobs[b].S : jobs[a].length > jobs[b].length;
  });
  uint32_t n64 = 0;
  std::vector<EncGatherTask> gather_tasks;
  size_t n_blocks_all = 0;
  for (uint32_t k : coded)
  {
    n64 += jobs[k].S == 64;
    const uint32_t parts = chain_gather_parts(jobs[k].slot_max);
    n_blocks_all += jobs[k].cb.size();
    if (gather_tasks.size() + jobs[k].cb.size() * parts >= kMaxTasks)
      return all_fail(members, count, out_dplans, HSRANS_E_ARG); // (nothing coded yet: no output byte changed)
    for (uint32_t b = 0; b < jobs[k].cb.size(); b++)
      for (uint32_t p = 0; p < parts; p++)
        gather_tasks.push_back(EncGatherTask{k, b, p, parts});
  }
  meta = Carve{};
  Carve scratch, ck;
  const size_t off_params2 = meta.take((size_t)count * sizeof(EncParams), 256);
  const size_t off_list = meta.take(coded.size() * 4, 256);
  const size_t off_gather = meta.take(gather_tasks.size() * sizeof(EncGatherTask), 256);
  std::vector<size_t> up_at(count), down_at(count), ck_at(count), scratch_at(count);
  for (uint32_t k : coded)
    up_at[k] = meta.take(chain_up_bytes(jobs[k]), 256);
  const size_t upload2_bytes = meta.at;
  const size_t off_down = meta.close();
  for (uint32_t k : coded)
    down_at[k] = meta.take(chain_down_bytes(jobs[k]), 256);
  const size_t down_bytes = meta.at - off_down;
  for (uint32_t k : coded)
    if (jobs[k].want_plan)
      ck_at[k] = ck.take(chain_ck_bytes(jobs[k]), 256);
  const size_t ck_down_bytes = ck.at;
  for (uint32_t k : coded)
  {
    if (!jobs[k].want_plan)
      ck_at[k] = ck.take(chain_ck_bytes(jobs[k]), 256);
    scratch_at[k] = scratch.take(jobs[k].slot_total, 512);
  }
  if (!encoder_buffers(ctx, scratch.at, meta.at, std::max<size_t>(ck.at, 256)))
    return all_fail(members, count, out_dplans, HSRANS_E_HIP);
  d_meta = ctx->d_enc_meta;
  upload.assign(upload2_bytes, 0);
  std::vector<uint8_t> down(down_bytes), ck_down(ck_down_bytes);
  {
    EncParams *params = (EncParams *)(upload.data() + off_params2);
    for (uint32_t k : coded)
    {
      params[k] = chain_params(jobs[k], ctx->d_enc_scratch + scratch_at[k], d_meta + down_at[k], d_meta + up_at[k], ctx->d_enc_ck + ck_at[k]);
      chain_up_fill(jobs[k], upload.data() + up_at[k]);
    }
    if (!coded.empty())
      memcpy(upload.data() + off_list, coded.data(), coded.size() * 4);
    if (!gather_tasks.empty())
      memcpy(upload.data() + off_gather, gather_tasks.data(), gather_tasks.size() * sizeof(EncGatherTask));
  }
  ok = coded.empty() ||
       (hipMemcpyAsync(d_meta, upload.data(), upload2_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
        launch_encode_chain_batch((const EncParams *)(d_meta + off_params2), (const uint32_t *)(d_meta + off_list), n64, (uint32_t)coded.size() - n64,
                                  (const EncGatherTask *)(d_meta + off_gather), (uint32_t)gather_tasks.size(), s, &launches) == hipSuccess &&
        hipMemcpyAsync(down.data(), d_meta + off_down, down_bytes, hipMemcpyDeviceToHost, s) == hipSuccess &&
        (ck_down_bytes == 0 || hipMemcpyAsync(ck_down.data(), ctx->d_enc_ck, ck_down_bytes, hipMemcpyDeviceToHost, s) == hipSuccess));
  if (!stream_settle(s, ok)) // (upload may be read until here)
    return all_fail(members, count, out_dplans, HSRANS_E_HIP);
  const auto t3 = std::chrono::steady_clock::now();

  // ---- d. results and plans: what came down through the single call's plan finish ----
  for (uint32_t k : coded)
  {
    const ChainJob &job = jobs[k];
    const uint8_t *dn = down.data() + (down_at[k] - off_down);
    const ChainDown at = chain_down_layout(job);
    const uint64_t *result = (const uint64_t *)(dn + at.result);
    if (!enc_result_ok(result, true))
    {
      member_fail(members, out_dplans, k, HSRANS_E_DEVICE);
      continue;
    }
    const size_t total = (size_t)result[0];
    if (job.want_plan)
    {
      const uint32_t *ck_states = (const uint32_t *)(ck_down.data() + ck_at[k]);
      const ChainCk ck = chain_ck_layout(job);
      hsrans_encode_opts *o = members[k].opts;
      const size_t psize = chain_plan_finish(job, total, (const uint64_t *)(dn + at.image_bytes), (const uint64_t *)(dn + at.image_off), ck_states + ck.block_states,
                                             ck_states, ck_states + ck.ck_pos, o->plan_out, o->plan_capacity);
      if (psize == 0)
      {
        member_fail(members, out_dplans, k, HSRANS_E_ARG);
        continue;
      }
      o->plan_size = psize;
      if (out_dplans != nullptr && hsrans_dplan_create(ctx, o->plan_out, psize, &out_dplans[k]) != HSRANS_OK)
      {
        out_dplans[k] = nullptr;
        member_fail(members, out_dplans, k, HSRANS_E_HIP);
        continue;
      }
    }
    members[k].stream_length = total;
  }
  for (uint32_t k = 0; k < count && rc == HSRANS_OK; k++)
    rc = members[k].rc;
  const auto t4 = std::chrono::steady_clock::now();
  if (stats)
  {
    stats->launches = launches;
    stats->blocks = (uint32_t)n_blocks_all;
    stats->summaries_us = us_between(t0, t1);
    stats->walk_us = us_between(t1, t2);
    stats->chain_us = us_between(t2, t3);
    stats->plans_us = us_between(t3, t4);
  }
  if (ctx->tuning.debug_stamps)
    fprintf(stderr, "[hsrans chain encode batch] members %u  blocks %zu  units %zu  summaries %.1f us  walks %.1f us  chain+gather %.1f us  plans %.1f us\n", count,
            n_blocks_all, n_unit_tasks, us_between(t0, t1), us_between(t1, t2), us_between(t2, t3), us_between(t3, t4));
  return rc;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI; thrown only after the caller's out_dplans was reset)
{
  return all_fail(members, count, out_dplans, HSRANS_E_HIP);
}
