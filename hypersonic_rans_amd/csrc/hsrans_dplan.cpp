// Device plans (hsrans_dplan, hsrans_internal.h): creation, (re)filling from a host plan blob, launch and release.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_host.h"
#include "hsrans_kernels.h"

using namespace hsrans;

#include "hsrans_internal.h"


extern "C"
{

// (Re)fills a device plan from a validated host plan blob: uploads it and prepares whatever the launch of this plan's
// kind needs (persistent arguments + host-built table, or the group list).  Device buffers are kept and grown, so a plan
// object can be refilled per call without allocations (the host-pointer entries do that).  The device must be current.

extern "C++" int dplan_fill(hsrans_dplan *d, const uint8_t *plan, size_t plan_size, const PlanHeader &h, hipStream_t s)
{
  hsrans_ctx *ctx = d->ctx;
  static_cast<DplanState &>(*d) = DplanState{};
  d->hdr = h;
  d->plan_bytes = plan_size;
  {
    d->out_hi = h.decoded_len;
    if (!(h.flags & kPlanWalk)) // (a walk plan starts from the states at stream + 16: body_lo stays 0)
    {
      const Piece *pc = (const Piece *)(plan + plan_pieces_off(h.n_chains));
      uint64_t lo = h.stream_len, olo = h.decoded_len, ohi = 0;
      for (uint32_t i = 0; i < h.n_pieces; i++)
      {
        const Piece &p = pc[i];
        const uint64_t len = (p.flags & kPieceFill) ? p.fill_len : (uint64_t)p.steps * h.states + p.tail;
        olo = std::min(olo, p.out_off);
        ohi = std::max(ohi, p.out_off + len);
        if (p.flags & kPieceFill)
          continue;
        lo = std::min(lo, p.words_off);
        if (!h.shared_hist || !(h.flags & kPlanHasHist)) // the kernel reads this histogram from the stream
          lo = std::min(lo, p.hist_off);
      }
      d->body_lo = lo;
      d->out_lo = std::min(olo, ohi);
      d->out_hi = ohi;
    }
  }
  // one allocation for everything this function uploads (sizes: upper bounds known from the header alone)
  const bool mergeable_raw = (h.flags & kPlanMergeable) && h.container == HSRANS_RAW;
  const bool may_group = !(h.flags & (kPlanWalk | kPlanMergeable)) && h.n_chains > 1;
  DplanRegions r;
  r.counters = (mergeable_raw && h.interval != 0) || may_group; // (one-chain-per-wave plans draw nothing)
  r.plan = plan_size;
  r.table = mergeable_raw && (h.flags & kPlanHasHist) ? std::max<size_t>((size_t)8 << h.bits, rank_table_entries(h.bits >= 13 ? h.bits : 13) * 8) : 0;
  r.groups = may_group ? ((size_t)h.n_chains + 16) * sizeof(Group) : 0;
  // status word and ticket counters start from zero on every (re)fill: "ticket mod draws-per-launch" only works while every
  // launch on a set of heads draws the same number of tickets, i.e. for ONE plan
  if (dplan_arena(d, r, s) != HSRANS_OK || hipMemcpyAsync(d->d_plan, plan, plan_size, hipMemcpyHostToDevice, s) != hipSuccess)
    return HSRANS_E_HIP;
  std::vector<uint2> tab;     // (host copies of what is uploaded asynchronously: alive until the one synchronisation at the end)
  std::vector<Group> groups;
  auto fail = [&](int rc) { // (nothing queued above may still be reading `plan`, `tab` or `groups` when the caller sees the failure)
    (void)hipStreamSynchronize(s);
    return rc;
  };
  if (mergeable_raw)
  {
    // persistent launch arguments, taken from the plan once (hsrans_kernels.h PersistentArgs).  plan_validate has
    // re-derived what the flag promises: single-piece chains, back to back in output and stream, tail on the last only,
    // uniform `interval` (or interval == 0: chains of any length, decoded one per wave by the direct launch)
    const Piece *pc = (const Piece *)(plan + plan_pieces_off(h.n_chains));
    const Piece &first = pc[0], &last = pc[h.n_pieces - 1];
    const uint64_t steps_total = (last.out_off - first.out_off) / h.states + last.steps;
    if (first.out_off > h.decoded_len || steps_total * h.states + last.tail > h.decoded_len - first.out_off)
      return fail(HSRANS_E_FORMAT);
    {
      uint64_t sig = 0x9E3779B97F4A7C15ull ^ ((uint64_t)h.states << 48) ^ ((uint64_t)h.bits << 40) ^ h.n_chains;
      for (uint32_t i = 0; i < h.n_pieces; i++)
        sig = (sig ^ pc[i].steps) * 0x100000001B3ull + (sig >> 29);
      d->deal_sig = sig ? sig : 1;
    }
    d->pa.pieces = (const Piece *)(d->d_plan + plan_pieces_off(h.n_chains));
    d->pa.states = (const uint32_t *)(d->d_plan + plan_states_off(h.n_chains, h.n_pieces));
    d->pa.n_chains = h.n_chains;
    d->pa.interval = h.interval;
    d->pa.S = h.states;
    d->pa.bits = h.bits;
    d->pa.out_base = first.out_off;
    d->pa.steps_total = steps_total;
    d->pa.hist_off = h.aux_off;
    d->pa.tail = last.tail;
    d->pa.counters = d->d_counters;
    if (h.flags & kPlanHasHist)
    {
      const uint16_t *counts = (const uint16_t *)(plan + plan_hist_off(h.n_chains, h.n_pieces, h.states));
      TableChoice tc = choose_table(d->tuning, h.bits, h.states, h.interval == 0);
      if (tc.dual)
      {
        // k_decode_dual reads the two neighbouring chains of a wave through ONE 32-bit window of the stream: a pair whose words
        // could span 4 GiB (a multi-GiB stream indexed for very few chains, e.g. by hsrans_plan_thin) goes one chain per wave
        for (uint32_t a = 0; a < h.n_chains && tc.dual; a += 2)
          if ((a + 2 < h.n_chains ? pc[a + 2].words_off : h.stream_len) - pc[a].words_off >= 0xFFFF0000ull)
            tc = choose_table(d->tuning, h.bits, h.states, false);
      }
      uint32_t mode = tc.mode;
      if (mode == 3 || mode == 5)
      {
        // decode table for the shared-table kernel (MODE 3): {freq | sym << 24, slot - cumul} per slot, the same
        // entries build_table<kModePack64> produces (hist.cpp:291-306 / :308-324 for the sum check)
        const uint32_t total = 1u << h.bits;
        tab.resize(total);
        uint32_t cum = 0;
        for (uint32_t sy = 0; sy < 256; sy++)
        {
          for (uint32_t k = 0; k < counts[sy] && cum + k < total; k++)
            tab[cum + k] = make_uint2((uint32_t)counts[sy] | (sy << 24), k);
          cum += counts[sy];
        }
        if (cum != total)
          return fail(HSRANS_E_FORMAT);
      }
      else if (mode == 4)
      {
        // wider histograms: the rank table (kModeRank: a byte per slot + 256 entries), 18 / 34 KiB at 14 / 15 bits instead of 128 / 256 KiB
        tab.resize(rank_table_entries(h.bits));
        if (build_rank_table(counts, h.bits, tab.data(), tab.size()) == 0)
          return fail(HSRANS_E_FORMAT);
      }
      d->pa.dual = tc.dual ? 1 : 0;
      if (mode != 0)
      {
        if (tab.size() * sizeof(uint2) > r.table || hipMemcpyAsync(d->d_table, tab.data(), tab.size() * sizeof(uint2), hipMemcpyHostToDevice, s) != hipSuccess)
          return fail(HSRANS_E_HIP);
        d->pa.table = (const uint2 *)d->d_table;
        d->pa.table_mode = mode;
        d->pa.hist_copy = (const uint16_t *)(d->d_plan + plan_hist_off(h.n_chains, h.n_pieces, h.states));
      }
    }
  }
  if (h.shared_hist && d->pa.table == nullptr) // no host-built table: the kernel builds its own from the histogram in the stream
    d->body_lo = std::min(d->body_lo, h.aux_off);
  if (h.container == HSRANS_RAW && h.n_chains == 1 && h.n_pieces == 1 && !(h.flags & kPlanWalk) && h.bits <= 14)
  {
    // a raw stream without an index: one chain — the two-wave latency kernel (k_decode_single) instead of one wave of k_decode
    const Piece &p = *(const Piece *)(plan + plan_pieces_off(1));
    if (!(p.flags & kPieceFill))
    {
      d->single.valid = 1;
      d->single.steps = p.steps;
      d->single.tail = p.tail;
      d->single.S = h.states;
      d->single.bits = h.bits;
      d->single.ring_entries = h.bits <= 13 ? 2048 : 1024; // 14 bits: 128 KiB of table leave room for 1,088 ring entries
      d->single.hist_off = p.hist_off;
      d->single.words_off = p.words_off;
      d->single.out_off = p.out_off;
    }
  }
  if (!(h.flags & (kPlanWalk | kPlanMergeable)) && h.n_chains > 1)
  {
    // group consecutive chains that decode with the same histogram (= the chains of one block_/mt_ block)
    const uint32_t *cf = (const uint32_t *)(plan + plan_chain_first_off());
    const Piece *pc = (const Piece *)(plan + plan_pieces_off(h.n_chains));
    for (uint32_t ch = 0; ch < h.n_chains; ch++)
    {
      const Piece &p = pc[cf[ch]];
      const bool single = cf[ch + 1] - cf[ch] == 1;
      const bool fill = (p.flags & kPieceFill) != 0;
      bool joins = false;
      if (!groups.empty() && single)
      {
        Group &g = groups.back();
        const Piece &q = pc[cf[ch - 1]];
        if (fill && (g.flags & kGroupFill))
          joins = true;
        else if (!fill && !(g.flags & kGroupFill) && g.hist_off == p.hist_off)
        {
          joins = true;
          if (!(cf[ch] - cf[ch - 1] == 1 && q.tail == 0 && q.out_off + (uint64_t)q.steps * h.states == p.out_off && q.words_off <= p.words_off && p.state_idx == ch))
            g.flags &= ~kGroupMergeable;
        }
      }
      if (joins)
        groups.back().count++;
      else
      {
        Group g{};
        g.begin = ch;
        g.count = 1;
        g.flags = fill ? kGroupFill : (single && p.state_idx == ch ? kGroupMergeable : 0);
        g.piece0 = cf[ch];
        g.hist_off = fill ? 0 : p.hist_off;
        g.words_end = h.stream_len;
        // the previous rANS group's words end no later than this group's histogram / header
        if (!fill && !groups.empty())
          for (size_t k = groups.size(); k-- > 0 && groups[k].words_end == h.stream_len;)
            groups[k].words_end = p.hist_off;
        groups.push_back(g);
      }
    }
    // Few, large blocks: mergeable groups are cut into parts (group_parts_max).  A part is a group of its own: same histogram, a
    // sub-range of the chains, and its words end where the next part's first chain starts reading.
    // k_decode_spread (all chains dealt out over every resident wave, kernels_spread.h) wants single-piece chains — chain c is piece
    // c with states c — and no share of the chains touching three blocks: the launcher compares its longest share with the fewest
    // chains of a coded block that is not the last
    {
      bool ok = h.states == 64 && h.n_pieces == h.n_chains && groups.size() < h.n_chains;
      size_t last_coded = groups.size(), first_coded = groups.size();
      for (size_t k = groups.size(); k-- > 0 && last_coded == groups.size();)
        if (!(groups[k].flags & kGroupFill))
          last_coded = k;
      for (size_t k = 0; k < groups.size() && first_coded == groups.size(); k++)
        if (!(groups[k].flags & kGroupFill))
          first_coded = k;
      // (a share touches three coded blocks only when one lies wholly INSIDE it: neither the plan's first nor its last coded block can —
      // a slice of a plan, e.g. a rank's run of a sharded decode, usually begins and ends with part of a block)
      uint32_t fewest = 0xFFFFFFFFu;
      for (size_t k = 0; k < groups.size() && ok; k++)
      {
        const Group &g = groups[k];
        if (g.flags & kGroupFill)
          continue;
        ok = (g.flags & kGroupMergeable) && g.piece0 == g.begin;
        if (k != last_coded && k != first_coded)
          fewest = std::min(fewest, g.count);
      }
      d->spread_min_block = ok ? fewest : 0;
      // k_decode_dealt: the blocks as chain ranges, where every one of them is a coded block of such chains
      bool plain = ok && !groups.empty();
      for (size_t k = 0; k < groups.size() && plain; k++)
        plain = !(groups[k].flags & kGroupFill) && groups[k].begin == (k ? groups[k - 1].begin + groups[k - 1].count : 0);
      if (plain)
      {
        d->block_begin.reserve(groups.size() + 1);
        for (const Group &g : groups)
          d->block_begin.push_back(g.begin);
        d->block_begin.push_back(h.n_chains);
      }
    }
    const uint32_t k_max = group_parts_max(ctx->geom, groups.size());
    if (groups.size() < h.n_chains && k_max > 1)
    {
      std::vector<Group> parts;
      for (const Group &g : groups)
      {
        const uint32_t k = (g.flags & kGroupMergeable) ? group_parts_of(g.count, k_max) : 1;
        if (k < 2)
        {
          parts.push_back(g);
          continue;
        }
        for (uint32_t part = 0; part < k; part++)
        {
          Group q = g;
          const uint32_t lo = (uint32_t)((uint64_t)g.count * part / k), hi = (uint32_t)((uint64_t)g.count * (part + 1) / k);
          q.begin = g.begin + lo;
          q.piece0 = g.piece0 + lo;
          q.count = hi - lo;
          if (part + 1 < k)
            q.words_end = pc[cf[g.begin + hi]].words_off;
          parts.push_back(q);
        }
      }
      groups.swap(parts);
    }
    // (Dynamic group order, run_grouped: the END of the list decides how evenly the launch finishes.  Cutting the last eighth /
    // quarter of the list into half-blocks was built and measured in round 3 at 2^30 bytes — 0.454-0.458 ms against 0.451-0.456
    // without: the extra table builds cost what the evener finish gains — and is gone.)
    if (!d->part_ends.empty() && d->part_ends.size() <= kMaxLaunchParts)
    {
      // the sub-runs of a sharded decode (hsrans_comm.cpp): which of them a group overlaps, and how many groups each will be counted by
      const std::vector<uint32_t> &ends = d->part_ends;
      auto part_of = [&](uint32_t chain) { return (uint32_t)(std::upper_bound(ends.begin(), ends.end(), chain) - ends.begin()); };
      d->part_units.assign(ends.size(), 0);
      d->part_cum.assign(ends.size(), 0);
      for (Group &g : groups)
      {
        const uint32_t lo = std::min<uint32_t>(part_of(g.begin), (uint32_t)ends.size() - 1), hi = std::min<uint32_t>(part_of(g.begin + g.count - 1), (uint32_t)ends.size() - 1);
        g.flags = (g.flags & ((1u << kGroupPartShift) - 1)) | (lo << kGroupPartShift) | (hi << (kGroupPartShift + 8));
        for (uint32_t p = lo; p <= hi; p++)
          d->part_units[p]++;
      }
    }
    if (groups.size() < h.n_chains)
    {
      // (the dynamic group order's ticket counters: d_counters, zeroed above)
      if (groups.size() * sizeof(Group) > r.groups || hipMemcpyAsync(d->d_groups, groups.data(), groups.size() * sizeof(Group), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(HSRANS_E_HIP);
      d->n_groups = (uint32_t)groups.size();
      d->groups_lean = h.states == 64;
      for (const Group &g : groups)
        if (!(g.flags & (kGroupMergeable | kGroupFill)))
          d->groups_lean = false;
    }
  }
  // `tab` and `groups` are about to go away: everything queued above has to have left them
  if (hipStreamSynchronize(s) != hipSuccess)
    return HSRANS_E_HIP;
  return HSRANS_OK;
}

// Plans written on the device (the GPU encoder's, an indexing decode's) have their group list there: a block's parts are consecutive groups of one
// histogram.  One small copy (32 bytes a group) at plan creation gives k_decode_dealt's dealing the blocks as chain ranges.
static void dplan_blocks_from_device_groups(hsrans_dplan *d, hipStream_t s, const Group *host_groups)
{
  d->block_begin.clear();
  d->dealt_state = 0;
  if (d->n_groups == 0 || d->d_groups == nullptr || !d->groups_lean || d->hdr.n_pieces != d->hdr.n_chains)
    return;
  try
  {
    std::vector<Group> groups(d->n_groups);
    if (host_groups != nullptr) // (the caller brought them down already)
      memcpy(groups.data(), host_groups, groups.size() * sizeof(Group));
    else if (hipMemcpyAsync(groups.data(), d->d_groups, groups.size() * sizeof(Group), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    {
      (void)hipGetLastError();
      return;
    }
    std::vector<uint32_t> begins;
    uint32_t next = 0;
    for (size_t k = 0; k < groups.size(); k++)
    {
      const Group &g = groups[k];
      if (g.count == 0) // (device builders leave unused part slots empty)
        continue;
      if ((g.flags & kGroupFill) || !(g.flags & kGroupMergeable) || g.begin != next || g.piece0 != g.begin)
      {
        if (d->tuning.dealt_trace)
          fprintf(stderr, "hsrans dealt: group %zu of %zu: flags %x begin %u count %u piece0 %u, expected begin %u\n", k, groups.size(), g.flags, g.begin, g.count, g.piece0, next);
        return;
      }
      if (begins.empty() || g.hist_off != groups[k - 1].hist_off || groups[k - 1].count == 0)
      {
        // (a part continues its block when the previous non-empty group has the same histogram)
        bool cont = false;
        for (size_t j = k; j-- > 0;)
          if (groups[j].count != 0)
          {
            cont = groups[j].hist_off == g.hist_off;
            break;
          }
        if (!cont)
          begins.push_back(g.begin);
      }
      next = g.begin + g.count;
    }
    if (next != d->hdr.n_chains || begins.empty())
      return;
    begins.push_back(d->hdr.n_chains);
    d->block_begin.swap(begins);
  }
  catch (...)
  {
    d->block_begin.clear();
  }
}

extern "C++" int dplan_arena(hsrans_dplan *d, const DplanRegions &r, hipStream_t s, uint8_t **scratch)
{
  const size_t counter_bytes = r.counters ? (size_t)kCounterSets * kDynQueues * kDynQueueStride * 8 : 0;
  Carve at;
  at.take(256); // the status word
  at.take(counter_bytes);
  const size_t off_plan = at.take(r.plan), off_table = at.take(r.table), off_groups = at.take(r.groups), off_scratch = at.take(r.scratch);
  const size_t end = at.close();
  if (!grow(&d->d_arena, &d->d_arena_cap, end))
    return HSRANS_E_HIP;
  uint8_t *a = d->d_arena;
  d->d_status = (uint32_t *)a;
  d->d_counters = r.counters ? (unsigned long long *)(a + 256) : nullptr;
  d->d_plan = a + off_plan;
  d->d_table = r.table ? a + off_table : nullptr;
  d->d_groups = r.groups ? a + off_groups : nullptr;
  if (scratch)
    *scratch = r.scratch ? a + off_scratch : nullptr;
  d->epoch.store(0, std::memory_order_relaxed); // (the counters start from zero again)
  const size_t zero = r.zero == kZeroAll ? end : r.zero == kZeroThroughPlan ? off_plan + r.plan : off_plan;
  return hipMemsetAsync(a, 0, zero, s) == hipSuccess ? HSRANS_OK : HSRANS_E_HIP;
}

extern "C++" void dplan_adopt(hsrans_dplan *d, const PlanHeader &h, uint32_t n_groups, uint64_t spread_min_block, hipStream_t s, const Group *host_groups)
{
  d->tuning = read_tuning(); // (as a fill takes them)
  d->hdr = h;
  d->plan_bytes = (size_t)plan_size(h.n_chains, h.n_pieces, h.states, h.flags);
  d->out_hi = h.decoded_len; // a plan written on the device covers the whole stream and the whole output
  d->n_groups = n_groups;
  d->groups_lean = n_groups != 0 && h.states == 64; // (the device writes mergeable runs and fill groups only)
  d->spread_min_block = d->groups_lean ? (uint32_t)std::min<uint64_t>(spread_min_block, 0xFFFFFFFFu) : 0;
  if (n_groups == 0)
    d->d_groups = nullptr, d->d_counters = nullptr;
  dplan_blocks_from_device_groups(d, s, host_groups); // (k_decode_dealt's dealing wants the blocks as chain ranges: 32 bytes a group, once)
}

extern "C++" PlanHeader mt_plan_header(uint32_t states, uint32_t bits, uint64_t decoded_len, uint64_t stream_len, uint32_t n_chains)
{
  PlanHeader h{};
  memcpy(h.magic, "HSRPLAN1", 8);
  h.container = HSRANS_MT;
  h.states = states;
  h.bits = bits;
  h.decoded_len = decoded_len;
  h.stream_len = stream_len;
  h.n_chains = h.n_pieces = n_chains;
  return h;
}

extern "C++" hsrans_dplan *dplan_new(hsrans_ctx *ctx)
{
  hsrans_dplan *d = new (std::nothrow) hsrans_dplan;
  if (d == nullptr)
    return nullptr;
  d->ctx = ctx;
  if (d->tuning.debug_stamps && hipMalloc((void **)&d->d_stamps, kStampWaves * 8 * 8) == hipSuccess)
    (void)hipMemset(d->d_stamps, 0, kStampWaves * 8 * 8);
  return d;
}

// one launch of a filled device plan (asynchronous on s; the device must be current)
extern "C++" int dplan_launch(hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity, hipStream_t s, uint64_t stream_lo,
                              const PartArgs *part_words)
{
  KParams kp{};
  kp.stream = (const uint8_t *)d_stream;
  kp.stream_len = stream_length;
  kp.stream_lo = stream_lo;
  kp.out = (uint8_t *)d_out;
  kp.out_cap = out_capacity;
  kp.plan = d->d_plan;
  kp.status = d->d_status;
  kp.stamps = d->d_stamps;
  kp.finish = d->d_finish;
  kp.pa = d->pa;
  kp.single = d->single;
  kp.single_states = (const uint32_t *)(d->d_plan + plan_states_off(d->hdr.n_chains, d->hdr.n_pieces));
  if (kp.pa.counters != nullptr) // uniform persistent launch: its own set of queue heads
    kp.pa.counters += (size_t)(d->epoch.fetch_add(1, std::memory_order_relaxed) % kCounterSets) * kDynQueues * kDynQueueStride;
  if (d->n_groups)
  {
    kp.groups = (const Group *)d->d_groups;
    kp.n_groups = d->n_groups;
    kp.groups_lean = d->groups_lean ? 1 : 0;
    kp.spread = d->groups_lean ? d->spread_min_block : 0;
    kp.group_prio = d->tuning.group_prio;
    memcpy(kp.group_prio_class, d->tuning.group_prio_class, sizeof(kp.group_prio_class));
    // (requesting a round's records and first chunks before its table build: measured, no gain — the other workgroups of the CU
    // fill the gap either way — so off unless asked for)
    // dynamic group order: this launch's own ticket counter (the counter sets of the persistent launches, one head of each used)
    if (d->d_counters != nullptr && !d->tuning.group_static)
      kp.group_tickets = d->d_counters + (size_t)(d->epoch.fetch_add(1, std::memory_order_relaxed) % kCounterSets) * kDynQueues * kDynQueueStride;
  }
  // lean grouped plans of coded blocks: the host-dealt one-round launch where the plan suits it (dealt once per weight set)
  const DealtTable *dealt = nullptr;
  if (d->block_begin.size() >= 2 && dealt_eligible(d->tuning, d->hdr, d->ctx->geom, launch_facts(kp, nullptr, nullptr)))
  {
    uint32_t w8[8];
    const uint64_t total_groups = (d->out_hi - d->out_lo) / 64; // (what THIS plan's chains decode: a rank's slice of a sharded stream, not the stream)
    dealt_weights_now(d->tuning, d->ctx->geom, total_groups / ((uint64_t)spread_grid(d->ctx->geom) * 16), d->hdr.bits, w8);
    if (d->dealt_state == 0 || memcmp(w8, d->dealt_weights, sizeof(w8)) != 0)
      d->dealt_state = deal_shares(d->tuning, d->ctx->geom, d->block_begin.data(), (uint32_t)d->block_begin.size() - 1, d->hdr.n_chains, total_groups, d->hdr.bits, &d->dealt, d->dealt_weights) ? 1 : -1;
    if (d->dealt_state == 1)
      dealt = &d->dealt;
  }
  if (d->tuning.dealt_trace)
    fprintf(stderr, "hsrans dealt: groups %u lean %d blocks %zu bits %u chains %u state %d\n", d->n_groups, (int)d->groups_lean, d->block_begin.size(), d->hdr.bits, d->hdr.n_chains, d->dealt_state);
  if (part_words != nullptr)
  {
    // a rank's sub-runs in one launch: the caller's completion words and sequence number, this plan's parts and running totals
    if (d->part_ends.empty() || d->part_units.size() != d->part_ends.size() || d->n_groups == 0)
      return HSRANS_E_ARG;
    kp.parts = *part_words;
    PartPlan pp{(uint32_t)d->part_ends.size(), d->part_ends.data(), d->part_units.data(), d->part_cum.data()};
    return launch_decode(d->tuning, kp, d->hdr, d->ctx->geom, s, &d->info, &pp, dealt, d->dealt_weights) == hipSuccess ? HSRANS_OK : HSRANS_E_HIP;
  }
  return launch_decode(d->tuning, kp, d->hdr, d->ctx->geom, s, &d->info, nullptr, dealt, d->dealt_weights) == hipSuccess ? HSRANS_OK : HSRANS_E_HIP;
}

extern "C++" int dplan_create(hsrans_ctx *ctx, const uint8_t *plan, size_t plan_size, const std::vector<uint32_t> *part_ends, hsrans_dplan **out_dplan)
try
{
  if (ctx == nullptr || out_dplan == nullptr)
    return HSRANS_E_ARG;
  *out_dplan = nullptr;
  PlanHeader h;
  if (!read_header(plan, plan_size, &h) || !plan_validate(plan, plan_size, h.stream_len, h.decoded_len))
    return HSRANS_E_FORMAT;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hsrans_dplan *d = dplan_new(ctx);
  if (d == nullptr)
    return HSRANS_E_HIP;
  if (part_ends)
    d->part_ends = *part_ends;
  int rc = dplan_fill(d, plan, plan_size, h, nullptr);
  if (rc == HSRANS_OK && hipStreamSynchronize(nullptr) != hipSuccess)
    rc = HSRANS_E_HIP;
  if (rc != HSRANS_OK)
  {
    hsrans_dplan_destroy(d);
    return rc;
  }
  *out_dplan = d;
  return HSRANS_OK;
}
catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
{
  return HSRANS_E_HIP;
}

int hsrans_dplan_create(hsrans_ctx *ctx, const uint8_t *plan, size_t plan_size, hsrans_dplan **out_dplan)
{
  return dplan_create(ctx, plan, plan_size, nullptr, out_dplan);
}

int hsrans_dplan_create_from_device_stream(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_stream, size_t stream_length,
                                           size_t out_capacity, void *hip_stream, hsrans_dplan **out_dplan)
{
  // K2: the mt_ header chain is followed on the device, so a stream that only exists in HBM can be
  // planned without a host copy.  Pass 1 is a pointer chase by one wavefront (one 16-byte read per block: about one memory
  // round trip each) that lists the blocks; pass 2 writes the plan, one wavefront per block.
  if (ctx == nullptr || out_dplan == nullptr || d_stream == nullptr)
    return HSRANS_E_ARG;
  *out_dplan = nullptr;
  if ((container != HSRANS_MT && container != HSRANS_BLOCK) || !valid_codec(container, states, bits) || ((uintptr_t)d_stream & 15) != 0)
    return HSRANS_E_ARG;
  if (hipSetDevice(ctx->device) != hipSuccess)
    return HSRANS_E_HIP;
  hipStream_t s = (hipStream_t)hip_stream;
  if (container == HSRANS_BLOCK)
  try
  {
    // a block_ stream's inline headers are only found by decoding: its plan is the walk plan, and the host planner makes that from the
    // stream's head alone — the two lengths and the start states, 16 + 4 * states bytes — with the checks hsrans_plan_build makes
    const size_t head_bytes = 16 + 4 * (size_t)states;
    if (stream_length < head_bytes)
      return HSRANS_E_FORMAT;
    uint8_t head[16 + 4 * 64];
    if (hipMemcpyAsync(head, d_stream, head_bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return HSRANS_E_HIP;
    std::vector<uint8_t> plan;
    if (!plan_build_vec(container, states, bits, head, stream_length, out_capacity, &plan)) // (reads no byte behind the head of a block_ stream)
      return HSRANS_E_FORMAT;
    return hsrans_dplan_create(ctx, plan.data(), plan.size(), out_dplan);
  }
  catch (...) // (std::bad_alloc and friends: nothing is thrown across the C ABI)
  {
    return HSRANS_E_HIP;
  }
  WalkResult *d_res = nullptr;
  uint64_t *d_blocks = nullptr;
  WalkResult res{};
  hsrans_dplan *d = nullptr;
  int rc = HSRANS_E_HIP;
  do
  {
    if (hipMalloc((void **)&d_res, sizeof(WalkResult)) != hipSuccess)
      break;
    // block list: sized for blocks of >= 4 KiB on average, enlarged (up to one entry per 8 stream bytes, the smallest
    // block there is) when the chase reports that it ran out
    uint64_t max_blocks = out_capacity / 4096 + 4096;
    const uint64_t hard_max = std::min<uint64_t>(stream_length / 8 + 1, 0xFFFFFFFFull);
    bool chased = false;
    while (true)
    {
      max_blocks = std::min(max_blocks, hard_max);
      if (d_blocks)
        (void)hipFree(d_blocks);
      d_blocks = nullptr;
      if (hipMalloc((void **)&d_blocks, max_blocks * 16) != hipSuccess)
        break;
      if (launch_mt_chase((const uint8_t *)d_stream, stream_length, out_capacity, (uint32_t)states, d_blocks, (uint32_t)max_blocks, d_res, s) != hipSuccess ||
          hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        break;
      if (res.error == 7 && max_blocks < hard_max)
      {
        max_blocks *= 8;
        continue;
      }
      chased = true;
      break;
    }
    if (!chased)
      break;
    if (res.error != 0 || res.n_chains == 0)
    {
      rc = HSRANS_E_FORMAT;
      break;
    }
    d = dplan_new(ctx);
    if (d == nullptr)
      break;
    const PlanHeader h = mt_plan_header((uint32_t)states, bits, res.decoded_len, stream_length, res.n_chains);
    DplanRegions r;
    r.plan = (size_t)plan_size(h.n_chains, h.n_pieces, h.states, 0);
    r.zero = kZeroThroughPlan;
    WalkResult res2{};
    if (dplan_arena(d, r, s) != HSRANS_OK || hipMemcpyAsync(d->d_plan, &h, sizeof(h), hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_mt_fill((const uint8_t *)d_stream, stream_length, (uint32_t)states, bits, d_blocks, d->d_plan, h.n_chains, res.decoded_len, d_res, s) != hipSuccess ||
        hipMemcpyAsync(&res2, d_res, sizeof(res2), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      break;
    if (res2.error != 0)
    {
      rc = HSRANS_E_FORMAT;
      break;
    }
    dplan_adopt(d, h, 0, 0, s);
    rc = HSRANS_OK;
  } while (false);
  if (d_res)
    (void)hipFree(d_res);
  if (d_blocks)
    (void)hipFree(d_blocks);
  if (rc != HSRANS_OK)
  {
    hsrans_dplan_destroy(d);
    return rc;
  }
  *out_dplan = d;
  return HSRANS_OK;
}

size_t hsrans_dplan_read_plan(hsrans_dplan *d, uint8_t *out, size_t capacity)
{
  if (d == nullptr || out == nullptr || d->d_plan == nullptr || d->plan_bytes == 0 || capacity < d->plan_bytes)
    return 0;
  return hipMemcpy(out, d->d_plan, d->plan_bytes, hipMemcpyDeviceToHost) == hipSuccess ? d->plan_bytes : 0;
}

void hsrans_dplan_destroy(hsrans_dplan *d)
{
  if (d == nullptr)
    return;
  if (d->d_stamps)
    (void)hipFree(d->d_stamps);
  if (d->d_arena) // (status, counters, plan, table and groups live inside it)
    (void)hipFree(d->d_arena);
  delete d;
}

} // extern "C"
