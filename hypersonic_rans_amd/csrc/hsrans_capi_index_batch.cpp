// hsrans_capi_index_batch.cpp — hsrans_decode_device_indexing_batch: the first decode of many streams in one call.  The walks of block_ streams and
// the blocks of mt_ base plans are wavefront tasks of at most three launches (k_index_pass_batch, one per private table layout); behind them one
// count and one fill launch per kind write every member's indexed plan; one synchronisation brings all results and status words down.
// Part of the C ABI of libhsrans_hip.so (include/hsrans_hip.h).  What it shares with the single call is in hsrans_internal.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"

namespace
{

// a member between validation and adoption
struct Member
{
  bool walk = false;
  uint32_t local = 0; // its index among the members of its kind (mt_ members first in the result and status arrays)
  WalkAssemblySizes wz{};
  MtAssemblySizes mz{};
  uint32_t min_chains = 0, max_chains = 0, max_groups = 0;
  size_t ck_off = 0;     // its checkpoints in ctx->d_enc_ck
  size_t groups_off = 0; // its group list in the page-locked staging (64 states: dplan_adopt reads it)
  bool groups_down = false;
  hsrans_dplan *nd = nullptr;
  uint8_t *scratch = nullptr;
};

int refuse(hsrans_indexing_member *members, uint32_t count, int rc)
{
  for (uint32_t k = 0; k < count; k++)
    members[k].rc = rc, members[k].indexed = nullptr;
  return rc;
}

} // namespace

extern "C" int hsrans_decode_device_indexing_batch(hsrans_ctx *ctx, hsrans_indexing_member *members, uint32_t count, void *hip_stream, hsrans_indexing_batch_stats *stats)
try
{
  if (stats != nullptr)
    *stats = hsrans_indexing_batch_stats{};
  if (ctx == nullptr || members == nullptr || count == 0 || count > 65536)
    return HSRANS_E_ARG;

  for (uint32_t k = 0; k < count; k++) // (until a member's own result is known)
    members[k].rc = HSRANS_E_HIP, members[k].indexed = nullptr;

  // ---- validation: every member by the single call's rules, then the rules of the batch; nothing is launched or allocated before all passed ----
  std::vector<Member> ms(count);
  uint32_t n_walk = 0, n_mt = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    const hsrans_indexing_member &m = members[k];
    int rc = indexing_args_check(ctx, m.dplan, m.d_stream, m.stream_length, m.d_out, m.out_capacity, m.index_interval);
    if (rc == HSRANS_OK)
    {
      const PlanHeader &h = m.dplan->hdr;
      Member &e = ms[k];
      e.walk = (h.flags & kPlanWalk) != 0;
      // raw members — and whatever else the single call assembles on the host — gain nothing from the batch
      if (!e.walk && (!indexing_mt_on_device(h) || h.n_chains == 0))
        rc = HSRANS_E_ARG;
      else if (e.walk)
      {
        if (!walk_assembly_sizes(h, m.index_interval, &e.wz))
          rc = HSRANS_E_FORMAT;
        e.min_chains = 1;
        e.max_chains = (uint32_t)e.wz.max_chains;
        e.max_groups = (uint32_t)e.wz.max_groups;
        e.local = n_walk++;
      }
      else
      {
        e.mz = mt_assembly_sizes(ctx, h, m.index_interval);
        e.min_chains = h.n_chains;
        e.max_chains = e.mz.max_chains;
        e.max_groups = e.mz.max_groups;
        e.local = n_mt++;
      }
    }
    if (rc != HSRANS_OK)
      return refuse(members, count, rc);
  }
  {
    std::vector<const hsrans_dplan *> plans(count);
    for (uint32_t k = 0; k < count; k++)
      plans[k] = members[k].dplan;
    std::sort(plans.begin(), plans.end());
    // the overlap rule over what the kernels touch: outputs [d_out, d_out + decoded_len) are written, streams [d_stream, d_stream + stream_length) read
    std::vector<Span> spans;
    spans.reserve(2 * (size_t)count);
    for (uint32_t k = 0; k < count; k++)
    {
      const hsrans_indexing_member &m = members[k];
      spans.push_back({(uintptr_t)m.d_out, (uintptr_t)m.d_out + (uintptr_t)m.dplan->hdr.decoded_len, true});
      spans.push_back({(uintptr_t)m.d_stream, (uintptr_t)m.d_stream + m.stream_length, false});
    }
    if (std::adjacent_find(plans.begin(), plans.end()) != plans.end() || !spans_disjoint(spans))
      return refuse(members, count, HSRANS_E_ARG);
  }

  std::lock_guard<std::mutex> guard(ctx->lock);
  if (ctx->tuning.index_assemble_on_host)
  {
    // the comparison path: the single call's body, member by member
    int first = HSRANS_OK;
    for (uint32_t k = 0; k < count; k++)
    {
      hsrans_indexing_member &m = members[k];
      m.indexed = nullptr;
      m.rc = decode_device_indexing_impl(ctx, m.dplan, m.d_stream, m.stream_length, m.d_out, m.out_capacity, m.index_interval, hip_stream, &m.indexed, true);
      if (first == HSRANS_OK)
        first = m.rc;
    }
    if (stats != nullptr)
      stats->walk_members = n_walk, stats->mt_members = n_mt;
    return first;
  }
  if (hipSetDevice(ctx->device) != hipSuccess)
    return refuse(members, count, HSRANS_E_HIP);
  hipStream_t s = (hipStream_t)hip_stream;

  // ---- the tasks of the recording pass, by table layout and by descending work: the decoded bytes of a walk, of an mt_ block its member's
  // average (the blocks' own lengths are in the base plan, which is on the device) ----
  struct Task
  {
    uint32_t mode;
    uint64_t work;
    IndexPassTask t;
  };
  std::vector<Task> tasks;
  uint64_t n_tasks64 = 0;
  for (uint32_t k = 0; k < count; k++)
    n_tasks64 += ms[k].walk ? 1 : members[k].dplan->hdr.n_chains;
  if (n_tasks64 > 0x7FFFFFFFu)
    return refuse(members, count, HSRANS_E_ARG);
  tasks.reserve((size_t)n_tasks64);
  uint32_t mode_bits[kIndexPassModes] = {};
  for (uint32_t k = 0; k < count; k++)
  {
    const PlanHeader &h = members[k].dplan->hdr;
    const uint32_t mode = (uint32_t)index_pass_mode(h.bits), n = ms[k].walk ? 1 : h.n_chains;
    mode_bits[mode] = std::max(mode_bits[mode], h.bits);
    for (uint32_t c = 0; c < n; c++)
      tasks.push_back({mode, h.decoded_len / n, {k, c}});
  }
  std::sort(tasks.begin(), tasks.end(), [](const Task &a, const Task &b) {
    return a.mode != b.mode ? a.mode < b.mode : a.work != b.work ? a.work > b.work : a.t.member != b.t.member ? a.t.member < b.t.member : a.t.chain < b.t.chain;
  });
  const uint32_t n_tasks = (uint32_t)tasks.size();

  // ---- memory: the checkpoints of all members out of ctx->d_enc_ck, every member's new plan (its arena also holds a walk's records), the tables
  // the kernels read and the words they leave in ctx->d_enc_meta, the page-locked staging of both in ctx->h_pin ----
  Carve ck;
  for (uint32_t k = 0; k < count; k++)
  {
    const PassBytes &pb = ms[k].walk ? ms[k].wz.pbytes : ms[k].mz.pbytes;
    ms[k].ck_off = ck.take(pb.st + pb.wd);
  }
  const size_t ck_total = ck.close();
  // device: [IndexPassMember x count | tasks | IndexArgs x n_mt | WalkIndexArgs x n_walk | status words' addresses x count] up, [IndexResult x count | status x count] down
  Carve at; // (the page-locked staging: the same, then the group lists that come down)
  at.take((size_t)count * sizeof(IndexPassMember));
  const size_t off_tasks = at.take((size_t)n_tasks * sizeof(IndexPassTask)), off_ia = at.take((size_t)n_mt * sizeof(IndexArgs));
  const size_t off_wa = at.take((size_t)n_walk * sizeof(WalkIndexArgs)), off_ptr = at.take((size_t)count * sizeof(uint32_t *)), up_bytes = at.close();
  const size_t off_res = at.take((size_t)count * sizeof(IndexResult)), off_status = at.take((size_t)count * 4), down_bytes = at.close() - off_res;
  for (uint32_t k = 0; k < count; k++)
    if (members[k].dplan->hdr.states == 64 && ms[k].max_groups != 0)
    {
      ms[k].groups_down = true;
      ms[k].groups_off = at.take((size_t)ms[k].max_groups * sizeof(Group));
    }
  const size_t pin_bytes = at.close();
  if (!grow(&ctx->d_enc_ck, &ctx->d_enc_ck_cap, ck_total) || !grow(&ctx->d_enc_meta, &ctx->d_enc_meta_cap, up_bytes + down_bytes) ||
      !grow_pinned(&ctx->h_pin, &ctx->h_pin_cap, pin_bytes))
    return refuse(members, count, HSRANS_E_HIP);
  uint8_t *dev = ctx->d_enc_meta, *pin = ctx->h_pin;

  const auto drop_plans = [&] {
    (void)hipStreamSynchronize(s); // (nothing queued here may still be running when a plan's arena is freed, or when the call returns)
    (void)hipGetLastError();
    for (Member &e : ms)
      if (e.nd != nullptr)
        hsrans_dplan_destroy(e.nd), e.nd = nullptr;
  };
  for (uint32_t k = 0; k < count; k++)
  {
    Member &e = ms[k];
    const PlanHeader &h = members[k].dplan->hdr;
    e.nd = e.walk ? assembly_plan(ctx, h.states, e.max_chains, e.max_groups, 2 * (size_t)e.wz.max_blocks, e.wz.pbytes.blk + e.wz.pbytes.bst, s, &e.scratch)
                  : assembly_plan(ctx, h.states, e.max_chains, e.max_groups, 2 * (size_t)h.n_chains, 0, s, &e.scratch);
    if (e.nd == nullptr)
    {
      drop_plans();
      return refuse(members, count, HSRANS_E_HIP);
    }
  }

  IndexPassMember *recs = (IndexPassMember *)pin;
  IndexPassTask *h_tasks = (IndexPassTask *)(pin + off_tasks);
  IndexArgs *h_ia = (IndexArgs *)(pin + off_ia);
  WalkIndexArgs *h_wa = (WalkIndexArgs *)(pin + off_wa);
  const uint32_t **h_ptr = (const uint32_t **)(pin + off_ptr); // mt_ members' first, then the walks'
  IndexResult *d_res = (IndexResult *)(dev + off_res);
  uint32_t most_base = 0, most_blocks = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    Member &e = ms[k];
    const hsrans_indexing_member &m = members[k];
    const hsrans_dplan *d = m.dplan;
    const PassBytes &pb = e.walk ? e.wz.pbytes : e.mz.pbytes;
    PassBuffers pass{};
    pass.ck_states = (uint32_t *)(ctx->d_enc_ck + e.ck_off);
    pass.ck_words = (uint64_t *)(ctx->d_enc_ck + e.ck_off + pb.st);
    const uint32_t slot = e.walk ? n_mt + e.local : e.local;
    if (e.walk)
    {
      walk_assembly_args(ctx, d, e.nd, e.scratch, m.index_interval, e.wz, &pass, &h_wa[e.local]);
      h_wa[e.local].result = d_res + slot;
      most_blocks = std::max(most_blocks, (uint32_t)e.wz.max_blocks);
    }
    else
    {
      mt_assembly_args(ctx, d, e.nd, e.scratch, m.index_interval, e.mz, pass, &h_ia[e.local]);
      h_ia[e.local].result = d_res + slot;
      most_base = std::max(most_base, d->hdr.n_chains);
    }
    h_ptr[slot] = d->d_status;
    IndexPassMember &r = recs[k];
    r = IndexPassMember{};
    r.stream = (const uint8_t *)m.d_stream;
    r.stream_len = m.stream_length;
    r.out = (uint8_t *)m.d_out;
    r.out_cap = m.out_capacity;
    r.plan = d->d_plan;
    r.status = d->d_status;
    r.ck_states = pass.ck_states;
    r.ck_words = pass.ck_words;
    r.walk_blocks = pass.walk_blocks;
    r.walk_states = pass.walk_states;
    r.walk_count = pass.walk_count;
    r.interval = m.index_interval;
    r.walk_max_blocks = pass.max_blocks;
  }
  for (uint32_t t = 0; t < n_tasks; t++)
    h_tasks[t] = tasks[t].t;

  // ---- the launches: the pass once per table layout present, count and fill once per kind; then everything the host needs, queued in front of
  // the one synchronisation ----
  uint32_t launches = 0;
  bool queued = hipMemcpyAsync(dev, pin, up_bytes, hipMemcpyHostToDevice, s) == hipSuccess && hipMemsetAsync(dev + off_res, 0, down_bytes, s) == hipSuccess;
  for (uint32_t t0 = 0; queued && t0 < n_tasks;)
  {
    uint32_t t1 = t0;
    while (t1 < n_tasks && tasks[t1].mode == tasks[t0].mode)
      t1++;
    queued = launch_index_pass_batch((int)tasks[t0].mode, mode_bits[tasks[t0].mode], (const IndexPassTask *)(dev + off_tasks) + t0, t1 - t0, (const IndexPassMember *)dev, s) == hipSuccess;
    launches++;
    t0 = t1;
  }
  const uint32_t *const *d_ptr = (const uint32_t *const *)(dev + off_ptr);
  uint32_t *d_status = (uint32_t *)(dev + off_status);
  if (queued && n_mt != 0)
  {
    queued = launch_index_assemble_batch((const IndexArgs *)(dev + off_ia), n_mt, most_base, d_ptr, d_status, s) == hipSuccess;
    launches += 2;
  }
  if (queued && n_walk != 0)
  {
    queued = launch_index_assemble_walk_batch((const WalkIndexArgs *)(dev + off_wa), n_walk, most_blocks, d_ptr + n_mt, d_status + n_mt, s) == hipSuccess;
    launches += 2;
  }
  queued = queued && hipMemcpyAsync(pin + off_res, dev + off_res, down_bytes, hipMemcpyDeviceToHost, s) == hipSuccess;
  for (uint32_t k = 0; queued && k < count; k++)
    if (ms[k].groups_down)
      queued = hipMemcpyAsync(pin + ms[k].groups_off, ms[k].nd->d_groups, (size_t)ms[k].max_groups * sizeof(Group), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (!queued || hipStreamSynchronize(s) != hipSuccess)
  {
    drop_plans();
    return refuse(members, count, HSRANS_E_HIP);
  }
  if (stats != nullptr)
  {
    stats->launches = launches;
    stats->walk_members = n_walk;
    stats->mt_members = n_mt;
    stats->tasks = n_tasks;
  }

  // ---- per member: its status word, its result against the bounds, its plan adopted ----
  const IndexResult *res = (const IndexResult *)(pin + off_res);
  const uint32_t *status = (const uint32_t *)(pin + off_status);
  bool clear = false, cleared = true;
  int first = HSRANS_OK;
  for (uint32_t k = 0; k < count; k++)
  {
    Member &e = ms[k];
    hsrans_indexing_member &m = members[k];
    const uint32_t slot = e.walk ? n_mt + e.local : e.local;
    int rc = HSRANS_OK;
    if (status[slot] != 0) // a bad histogram / header: reported and cleared like hsrans_dplan_status does
    {
      rc = HSRANS_E_DEVICE;
      clear = true;
      cleared = hipMemsetAsync(m.dplan->d_status, 0, 4, s) == hipSuccess && cleared;
    }
    m.rc = assembly_adopt(m.dplan, e.nd, rc, res[slot], m.index_interval, e.min_chains, e.max_chains, e.max_groups, s, e.groups_down ? (const Group *)(pin + e.groups_off) : nullptr);
    m.indexed = m.rc == HSRANS_OK ? e.nd : nullptr;
    e.nd = nullptr; // (adopted, or destroyed)
  }
  if (clear && !stream_settle(s, cleared))
  {
    for (uint32_t k = 0; k < count; k++)
      if (members[k].rc == HSRANS_E_DEVICE)
        members[k].rc = HSRANS_E_HIP;
  }
  for (uint32_t k = 0; k < count && first == HSRANS_OK; k++)
    first = members[k].rc;
  return first;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}
