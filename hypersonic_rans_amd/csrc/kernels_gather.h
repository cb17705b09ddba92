// kernels_gather.h — Random access: arbitrary byte ranges of one planned stream in one launch (hsrans_decode_device_gather, hsrans_decode_device_gather_indirect), and of many streams in one launch per table layout (hsrans_decode_device_gather_batch, hsrans_decode_device_gather_batch_indirect) — gather_groups, gather_tail, run_gather, gather_setup, k_gather, k_gather_cut, k_gather_ranges, k_gather_set, k_set_cut, k_set_ranges.
// Part of the one device translation unit hsrans_kernels.hip (which includes the parts in dependency order and holds the host-side launcher).
//
// One wavefront = one task (GatherTask: decoded bytes [begin, end) of the stream, destination = GatherParams::dst + byte + dst_delta).  The
// wave finds the last chain that starts at or before `begin` (binary search over the chains' first output bytes), enters it at its
// start states and decodes forward, chain after chain, until `end`: groups in front of `begin` are decoded and dropped, everything
// else is stored clipped to the task, and nothing outside [begin, end) is ever written.
// The four task kernels differ only in where a wave finds its task and its stream: each fills a GatherSource (from the launch's
// parameters, or from a gather set's member record), calls the one gather_setup and then run_gather.  The rules of a range
// (gather_range_ok, gather_range_tasks: hsrans_kernels.h) are the host entries' own functions, used by k_gather_cut and k_set_cut as they stand.
#ifndef HSRANS_KERNELS_GATHER_H
#define HSRANS_KERNELS_GATHER_H

namespace hsrans
{

// ring_advance for a loop that may not store at all: the wait that holds whatever else the wave has issued.  Younger than the request for
// chunk k + 1 are the requests for k + 2 .. k + HSRANS_RING_AHEAD (and perhaps a mirror: stricter), so "all but AHEAD - 1 done" implies it.
__device__ __forceinline__ void gather_advance(const StreamWin &sw, Ring &r, const WaveCtx &c)
{
  if ((r.cur >> (r.clog - 1)) > r.k)
  {
    r.k++;
    ring_request(sw, r, c, r.k + HSRANS_RING_AHEAD);
    if (HSRANS_RING_AHEAD == 3)
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  }
}

// `steps` whole groups of a piece whose next symbol is decoded byte o, clipped to [begin, end); stops behind the group that holds
// end - 1 (the wave has nothing more to decode then: its states are left mid-piece).  c.out is the task's destination of decoded byte 0.
//   in front of begin     decoded, nothing stored (the non-storing form of run_groups_impl's loop)
//   wholly inside         4 groups -> in-quad transpose -> one dword per lane, where the destination of the piece's groups is 4-byte
//                         aligned; else a byte per lane and group
//   the edges             a byte per lane under the lane's own test begin <= byte < end
template <int MODE, bool FULL>
__device__ __forceinline__ void gather_groups(uint32_t &x, const StreamWin &sw, Ring &r, const WaveCtx &c, uint64_t &o_ref, uint32_t steps, uint64_t begin, uint64_t end)
{
  uint64_t o = uni64(o_ref);
  const uint32_t S = FULL ? 64 : c.S;
  const bool act = FULL || c.lane < S;
  const unsigned long long act_mask = FULL ? ~0ull : __builtin_amdgcn_ballot_w64(act);
  constexpr uint32_t kSymByte = (MODE == kModePack64 || MODE == kModeRank || MODE == kModeSpill) ? 3 : 0;

  if (o + S <= begin)
  {
    const uint64_t in_front = groups_of(S, begin - o);
    uint32_t skip = in_front < steps ? (uint32_t)in_front : steps;
    steps -= skip;
    o += (uint64_t)skip * S;
    for (; skip >= 4; skip -= 4)
    {
      group_step<MODE, FULL>(x, r, c, act_mask);
      group_step<MODE, FULL>(x, r, c, act_mask);
      group_step<MODE, FULL>(x, r, c, act_mask);
      group_step<MODE, FULL>(x, r, c, act_mask);
      gather_advance(sw, r, c);
    }
    for (; skip > 0; skip--)
      group_step<MODE, FULL>(x, r, c, act_mask);
    gather_advance(sw, r, c);
  }

  const OutLanes ol = out_lanes(c.lane, S);
  const uint32_t p = lane_to_byte(c.lane);
  const bool aligned = uni((uint32_t)((uintptr_t)c.out + o) & 3u) == 0; // (S is a multiple of 4: the same for every group of the piece)
  while (steps > 0 && o < end)
  {
    if (aligned && steps >= 4 && o >= begin && o + 4 * S <= end)
    {
      const uint32_t e0 = group_step<MODE, FULL>(x, r, c, act_mask);
      const uint32_t e1 = group_step<MODE, FULL>(x, r, c, act_mask);
      const uint32_t e2 = group_step<MODE, FULL>(x, r, c, act_mask);
      const uint32_t e3 = group_step<MODE, FULL>(x, r, c, act_mask);
      const uint32_t acc = pack4<kSymByte>(e0, e1, e2, e3, ol);
      if (act)
        HSRANS_STORE_U32((uint32_t *)(c.out + o + ol.store_off), acc);
      o += 4 * S;
      steps -= 4;
    }
    else
    {
      const uint32_t e = group_step<MODE, FULL>(x, r, c, act_mask);
      const uint64_t b = o + p;
      if (act && b >= begin && b < end)
        c.out[b] = (uint8_t)(e >> (8 * kSymByte));
      o += S;
      steps--;
    }
    gather_advance(sw, r, c);
  }
  o_ref = o;
}

// the final masked group of a piece (run_tail), clipped
template <int MODE>
__device__ __forceinline__ void gather_tail(uint32_t &x, Ring &r, const WaveCtx &c, uint64_t o, uint32_t tail, uint64_t begin, uint64_t end)
{
  const uint32_t p = lane_to_byte(c.lane);
  const bool act = c.lane < c.S && p < tail;
  const uint32_t e = group_step<MODE, false>(x, r, c, __builtin_amdgcn_ballot_w64(act));
  const uint64_t b = o + p;
  if (act && b >= begin && b < end)
    c.out[b] = (uint8_t)(e >> ((MODE == kModePack64 || MODE == kModeRank || MODE == kModeSpill) ? 24 : 0));
}

// the task of one wave: decoded bytes [begin, end) go to dst + byte + dst_delta (all three wave-uniform).  SHARED: c.table holds the
// plan's one table already.  A wave may run task after task: nothing but the table of a SHARED launch is carried from one to the next.
template <int MODE, bool SHARED>
__device__ void run_gather(WaveCtx &c, const PlanView &pv, uint8_t *dst, uint64_t begin, uint64_t end, int64_t dst_delta)
{
  c.out = dst + dst_delta;
  const uint32_t n_chains = uni(pv.hdr->n_chains);
  if (begin >= end || n_chains == 0)
    return;
  // the last chain whose first output byte is <= begin (chain 0 where there is none: a plan that starts later writes nothing in front of itself)
  uint32_t lo = 0, hi = n_chains;
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (uni64(pv.pieces[uni(pv.chain_first[mid])].out_off) <= begin)
      lo = mid;
    else
      hi = mid;
  }
  uint32_t x = 0;
  uint64_t have_hist = ~(uint64_t)0, o = 0;
  bool live = false; // the ring stands right behind the last whole group of the piece before, whose decoding ended at output byte o
  StreamWin sw;
  Ring r;
  ring_bind(r, c.rings, 9, false);
  for (uint32_t chain = lo; chain < n_chains; chain++)
  {
    const uint32_t first = uni(pv.chain_first[chain]), last = uni(pv.chain_first[chain + 1]);
    for (uint32_t pi = first; pi < last; pi++)
    {
      const Piece *pc = pv.pieces + pi;
      const uint32_t flags = uni(pc->flags);
      const uint64_t out_off = uni64(pc->out_off);
      if (out_off >= end) // (pieces ascend in the output: nothing behind this one is the task's)
        return;
      if (flags & kPieceFill)
      {
        if (flags & kPieceChainStart)
          x = c.lane < c.S ? pv.states[(uint64_t)uni(pc->state_idx) * c.S + c.lane] : 0;
        const uint64_t f_end = out_off + uni64(pc->fill_len);
        const uint64_t f0 = out_off > begin ? out_off : begin, f1 = f_end < end ? f_end : end;
        if (f0 < f1)
          wave_fill(c, f0, f1 - f0, (uint32_t)uni64(pc->hist_off) & 0xFF);
        live = false;
        continue;
      }
      const uint64_t hist_off = uni64(pc->hist_off), words_off = uni64(pc->words_off);
      // a chain that starts exactly where this wave stands — same histogram, next output byte, next stream word — is the checkpoint of the
      // states the wave already holds: it decodes on without a new prologue (what kPlanMergeable promises of a whole plan, found per chain here)
      const bool cont = live && flags == kPieceChainStart && (SHARED || hist_off == have_hist) && out_off == o && words_off == ring_pos(sw, r);
      if (!cont)
      {
        if (flags & kPieceChainStart)
          x = c.lane < c.S ? pv.states[(uint64_t)uni(pc->state_idx) * c.S + c.lane] : 0;
        if (!SHARED && hist_off != have_hist)
        {
          if (uni(build_table<MODE, false>(c, hist_off, c.lane, 64) ? 1u : 0u) == 0) // (the same on every lane; said so, for the window and ring below live across this exit)
            return;
          have_hist = hist_off;
        }
        ring_init(sw, r, c, words_off, x);
      }
      o = out_off;
      if (c.S == 64)
        gather_groups<MODE, true>(x, sw, r, c, o, uni(pc->steps), begin, end);
      else
        gather_groups<MODE, false>(x, sw, r, c, o, uni(pc->steps), begin, end);
      if (o >= end)
        return;
      const uint32_t tail = uni(pc->tail);
      if (tail != 0)
        gather_tail<MODE>(x, r, c, o, tail, begin, end);
      live = tail == 0;
    }
  }
}

// what every gather kernel does before its first task: the wave's context and, in a SHARED launch, the workgroup's table.  gs, bits and
// states are wave-uniform, wave is the wave's number in its workgroup.  table_bytes: the table the LDS is laid out for (the plan's own;
// in a launch over many plans their largest), for a table per wave a multiple of 16.
// check_hist (SHARED; true in the workgroup's first wave at most, and gs.hist_copy / gs.hist_off are read there only): the wave checks
// that the stream carries the histogram the table was built from.
// A SHARED launch ends in a barrier: every wave of the workgroup comes here.
template <int MODE, bool SHARED>
__device__ __forceinline__ void gather_setup(WaveCtx &c, const GatherSource &gs, uint32_t bits, uint32_t states, uint32_t wave, uint32_t table_bytes, bool check_hist, uint8_t *smem)
{
  const uint32_t waves = blockDim.x >> 6;

  // (no output yet: run_gather sets it, task by task; no capacity: every store of these kernels is tested against its task)
  wave_ctx_begin(c, gs.stream, gs.stream_len, 0, nullptr, 0, gs.status, bits, states);

  if (SHARED)
  {
    wave_ctx_lds(c, smem, lds_layout_gather(MODE, table_bytes, waves), wave);
    c.gtable = gs.table;
    // the host-built table: one coalesced 16-byte load + LDS store per thread (none for the table that stays in global memory)
    // (copy_host_table, written out: the call changes the instruction sequences of k_gather<4, true> and k_gather_ranges<4, true>)
    const uint32_t entries = table_bytes_for(MODE, bits) / 8;
    for (uint32_t i = threadIdx.x * 2; i < entries; i += blockDim.x * 2)
      *(u32x4 *)(c.table + (uint64_t)i * 8) = *(const u32x4 *)(gs.table + i);
    if (check_hist)
      check_hist_copy<false>(c, gs.hist_copy, gs.hist_off);
    __syncthreads();
  }
  else
  {
    c.rings = smem + wave * kWaveRingBytes; // all rings first: they stay kRingBytes-aligned
    c.table = smem + waves * kWaveRingBytes + wave * table_bytes;
    c.table_b = c.table;
    c.gtable = nullptr;
    c.scratch_cnt = (uint16_t *)c.rings;
    c.scratch_cum = (uint16_t *)(c.rings + 512);
  }
}

// k_gather's and k_gather_ranges': one plan, whose header says bits and states; the launch's first workgroup checks the histogram
template <int MODE, bool SHARED>
__device__ __forceinline__ void gather_setup(WaveCtx &c, const PlanView &pv, const GatherParams &gp, uint8_t *smem)
{
  const uint32_t bits = pv.hdr->bits;
  const GatherSource gs{gp.plan, gp.status, gp.stream, gp.stream_len, gp.table, gp.hist_copy, gp.hist_off};
  const uint32_t table_bytes = table_bytes_for(MODE, bits);
  gather_setup<MODE, SHARED>(c, gs, bits, pv.hdr->states, uni(threadIdx.x >> 6), SHARED ? table_bytes : (table_bytes + 15) & ~15u, blockIdx.x == 0 && threadIdx.x < 64, smem);
}

// ---------------------------------------------------------------------------------------------------------------
// the kernel: blockDim.x = 64 * waves; wave w of block b runs task b * waves + w
// LDS: SHARED  -> [waves x ring][table] (the rank table first, as k_decode has it);   otherwise -> [waves x ring][waves x table]
// ---------------------------------------------------------------------------------------------------------------
template <int MODE, bool SHARED>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(80))) k_gather(GatherParams gp)
{
  extern __shared__ u32x4 smem_v[];
  const PlanView pv = plan_view(gp.plan);
  WaveCtx c;
  gather_setup<MODE, SHARED>(c, pv, gp, (uint8_t *)smem_v);
  const uint32_t task = blockIdx.x * (blockDim.x >> 6) + uni(threadIdx.x >> 6);
  if (task < gp.n_tasks)
    run_gather<MODE, SHARED>(c, pv, gp.dst, uni64(gp.tasks[task].begin), uni64(gp.tasks[task].end), (int64_t)uni64((uint64_t)gp.tasks[task].dst_delta));
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather_indirect: the ranges are in device memory and are read when the launch runs.  Two kernels, queued back to
// back: k_gather_cut checks the ranges and counts their tasks, k_gather_ranges runs them.
// Workspace (uint32 words; GatherWs* in hsrans_kernels.h): [0] the task total, 0 where anything was refused; [1] the ranges in use;
// from word kGatherWsFirst on first_task[0 .. n], the exclusive prefix of the ranges' task counts.
// ---------------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads, a range per thread and round.  The checks and the task count are the host entry's (gather_range_ok,
// gather_range_tasks: hsrans_kernels.h); one range that fails them, a count above max_count or a total of 2^31 or more refuses the whole call:
// the total is written as 0 and kStatusBadRange set.
__global__ void __launch_bounds__(1024) k_gather_cut(GatherCutParams cp)
{
  __shared__ uint64_t wave_sum[16];
  __shared__ uint32_t any_bad;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t *first_task = cp.workspace + kGatherWsFirst;
  uint32_t n = cp.count != nullptr ? *cp.count : cp.max_count;
  bool bad = n > cp.max_count;
  if (bad)
    n = 0;
  if (threadIdx.x == 0)
    any_bad = 0;
  __syncthreads();
  uint64_t carry = 0; // tasks of the rounds before this one (the same on every thread)
  for (uint32_t r0 = 0; r0 < n; r0 += 1024)
  {
    const uint32_t r = r0 + threadIdx.x;
    uint64_t tasks = 0;
    if (r < n)
    {
      const uint64_t offset = cp.ranges[r].offset, length = cp.ranges[r].length, dst_offset = cp.ranges[r].dst_offset;
      if (!gather_range_ok(offset, length, dst_offset, cp.decoded_len, cp.out_lo, cp.out_hi, cp.dst_capacity))
        bad = true;
      else
        tasks = gather_range_tasks(offset, length, cp.segment);
      if (tasks >= (1ull << 31)) // (so that no sum below can wrap)
      {
        bad = true;
        tasks = 0;
      }
    }
    // inclusive scan: inside the wave, then over the 16 waves' sums
    uint64_t incl = tasks;
    for (uint32_t d = 1; d < 64; d *= 2)
    {
      const uint64_t below = __shfl_up(incl, d, 64);
      if (lane >= d)
        incl += below;
    }
    __syncthreads(); // (wave_sum of the round before has been read)
    if (lane == 63)
      wave_sum[wave] = incl;
    __syncthreads();
    uint64_t before = carry, round = 0;
    for (uint32_t w = 0; w < 16; w++)
    {
      const uint64_t v = wave_sum[w];
      before += w < wave ? v : 0;
      round += v;
    }
    // (a prefix of 2^31 or more is refused below: what the low words then hold is never read)
    if (r < n)
      first_task[r] = (uint32_t)(before + incl - tasks);
    carry += round;
    if (carry >= (1ull << 31))
    {
      bad = true;
      carry = 1ull << 31;
    }
  }
  if (bad)
    any_bad = 1; // (benign race: every writer stores 1)
  __syncthreads();
  if (threadIdx.x == 0)
  {
    const bool refuse = any_bad != 0;
    first_task[n] = (uint32_t)carry;
    cp.workspace[kGatherWsTotal] = refuse ? 0 : (uint32_t)carry;
    cp.workspace[kGatherWsCount] = n;
    if (refuse)
      atomicOr(cp.status, kStatusBadRange);
  }
}

// blockDim.x = 64 * waves, any grid: wave w of block b runs tasks w * gridDim.x + b, + gridDim.x * waves, ... below the total that
// k_gather_cut left — neighbouring tasks go to different workgroups, so a total far below the grid's waves still spreads over the CUs
// (the grid is sized from max_count and dst_capacity, not from the ranges: gather_ranges_shape).  LDS as k_gather.
// (100 SGPRs: the loop keeps its own uniforms beside a task's; occupancy is the same 8 waves per SIMD)
template <int MODE, bool SHARED>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(100))) k_gather_ranges(GatherParams gp, GatherRangesParams rp)
{
  extern __shared__ u32x4 smem_v[];
  const uint32_t total = uni(rp.workspace[kGatherWsTotal]);
  if (blockIdx.x >= total) // (wave 0's first task is the workgroup's lowest: nothing for any of its waves, the table copy included)
    return;
  const PlanView pv = plan_view(gp.plan);
  WaveCtx c;
  gather_setup<MODE, SHARED>(c, pv, gp, (uint8_t *)smem_v);
  const uint32_t n = uni(rp.workspace[kGatherWsCount]);
  const uint32_t *first_task = rp.workspace + kGatherWsFirst;
  const uint32_t stride = gridDim.x * (blockDim.x >> 6);
  for (uint32_t t = uni(threadIdx.x >> 6) * gridDim.x + blockIdx.x; t < total; t += stride)
  {
    // the range of task t: the last r with first_task[r] <= t (ranges without tasks share their successor's entry and are passed over)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1)
    {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (uni(first_task[mid]) <= t)
        lo = mid;
      else
        hi = mid;
    }
    const uint64_t offset = uni64(rp.ranges[lo].offset), stop = offset + uni64(rp.ranges[lo].length), dst_offset = uni64(rp.ranges[lo].dst_offset);
    const uint64_t first_seg = rp.segment_shift != 0 ? offset >> rp.segment_shift : uni64(offset / rp.segment);
    const uint64_t cut = (first_seg + (t - uni(first_task[lo]))) * rp.segment;
    const uint64_t begin = cut > offset ? cut : offset, end = cut + rp.segment < stop ? cut + rp.segment : stop;
    run_gather<MODE, SHARED>(c, pv, gp.dst, begin, end, (int64_t)(dst_offset - offset));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather_batch: the tasks of many streams (the members of a gather set) whose gathers use one table layout, in one
// launch.  Every entry names its member; the wave takes stream, plan, status word, states and bits from the member's record (all
// wave-uniform) instead of from the launch's parameters, then runs its task as k_gather does.
// blockDim.x = 64 * waves; wave w of block b runs entry b * waves + w.
// SHARED: the host has sorted the entries by member and padded every member's run to a multiple of `waves` (hsrans_gather_batch_tasks),
// so a workgroup serves one member — that of its first entry — and copies that member's host-built table; the first workgroup of a
// member's run (the one before it serves another member, or there is none) checks that the member's stream carries the histogram the
// table was built from, as workgroup 0 of k_gather does.
// LDS as k_gather, with room for the largest table among the launch's members (sp.table_bytes) where k_gather has the plan's.
// ---------------------------------------------------------------------------------------------------------------
template <int MODE, bool SHARED>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(100))) k_gather_set(GatherSetParams sp)
{
  extern __shared__ u32x4 smem_v[];
  const uint32_t waves = blockDim.x >> 6;
  const uint32_t first = blockIdx.x * waves; // (< n_tasks: the grid is sized from the entries)
  const uint32_t wave = uni(threadIdx.x >> 6);
  const uint32_t entry = first + wave;
  if (!SHARED && entry >= sp.n_tasks) // (SHARED: the entries fill whole workgroups, and every wave must reach gather_setup's barrier)
    return;
  const GatherSetTask *task = sp.tasks + (SHARED && entry >= sp.n_tasks ? first : entry);
  const uint32_t member = uni(SHARED ? sp.tasks[first].member : task->member);
  const GatherSetMember *rec = sp.members + member;
  GatherSource gs{};
  gs.stream = (const uint8_t *)uni64((uint64_t)(uintptr_t)rec->src.stream);
  gs.stream_len = uni64(rec->src.stream_len);
  gs.plan = (const uint8_t *)uni64((uint64_t)(uintptr_t)rec->src.plan);
  gs.status = (uint32_t *)uni64((uint64_t)(uintptr_t)rec->src.status);
  // the first wave of the first workgroup of a member's run checks the histogram
  const bool check_hist = SHARED && threadIdx.x < 64 && (first == 0 || uni(sp.tasks[first - 1].member) != member);
  if (SHARED)
    gs.table = (const uint2 *)uni64((uint64_t)(uintptr_t)rec->src.table);
  if (check_hist)
  {
    gs.hist_copy = (const uint16_t *)uni64((uint64_t)(uintptr_t)rec->src.hist_copy);
    gs.hist_off = uni64(rec->src.hist_off);
  }
  const PlanView pv = plan_view(gs.plan);
  WaveCtx c;
  gather_setup<MODE, SHARED>(c, gs, uni(rec->bits), uni(rec->states), wave, sp.table_bytes, check_hist, (uint8_t *)smem_v);
  if (SHARED && entry >= sp.n_tasks)
    return;
  run_gather<MODE, SHARED>(c, pv, sp.dst, uni64(task->begin), uni64(task->end), (int64_t)uni64((uint64_t)task->dst_delta));
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather_batch_indirect: the ranges of many streams are in device memory and are read when the launches run.
// k_set_cut checks them, sorts them by their member's position (a counting sort: count, scan, scatter) and counts their tasks;
// one k_set_ranges per kind runs them.  Workspace: GatherSetWs (hsrans_kernels.h).
// ---------------------------------------------------------------------------------------------------------------
// The workspace words of k_set_cut are written and read again inside one launch, by different waves of its one workgroup: every such
// access goes to L2 (relaxed, agent scope — atomics are performed there, and a plain load could be served from a line this CU already
// holds), and set_cut_sync lets a wave's stores arrive before it joins the barrier.
__device__ __forceinline__ uint32_t set_ws_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void set_ws_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void set_cut_sync()
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
// exclusive prefix of v over the workgroup's 1024 threads, on top of `carry` (the sum of the rounds before, the same on every thread),
// which moves on by the round's sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ uint64_t set_cut_scan(uint64_t v, uint64_t *wave_sum, uint64_t &carry)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t incl = v;
  for (uint32_t d = 1; d < 64; d *= 2)
  {
    const uint64_t below = __shfl_up(incl, d, 64);
    if (lane >= d)
      incl += below;
  }
  __syncthreads(); // (wave_sum of the call before has been read)
  if (lane == 63)
    wave_sum[wave] = incl;
  __syncthreads();
  uint64_t before = carry, round = 0;
  for (uint32_t w = 0; w < 16; w++)
  {
    const uint64_t s = wave_sum[w];
    before += w < wave ? s : 0;
    round += s;
  }
  carry += round;
  return before + incl - v;
}
// One round of k_set_cut's passes over the ranges is kSetCutBatch rows per thread: the loads of a batch's rows are issued together, then
// those of their members' records — a pass is a chain of dependent loads, and a row at a time it would pay the chain once per 1024 rows.
constexpr uint32_t kSetCutBatch = 4;
// what the cut needs of a batch's rows: their tasks (0: none, or no row) and their members' positions; false: a row is refused (the host
// entry's rules: member, reserved, gather_range_ok, a range that has bytes on a member that cannot be cut, 2^31 tasks or more).
// No branch between the loads: rows beyond n read row 0, a member beyond the set reads the last record, and neither counts.
__device__ __forceinline__ bool set_cut_rows(const GatherSetCutParams &cp, uint64_t r0, uint32_t n, uint32_t (&tasks)[kSetCutBatch], uint32_t (&pos)[kSetCutBatch])
{
  GatherSetRange g[kSetCutBatch];
  uint64_t segment[kSetCutBatch], decoded_len[kSetCutBatch], out_lo[kSetCutBatch], out_hi[kSetCutBatch];
  bool in[kSetCutBatch];
#pragma unroll
  for (uint32_t j = 0; j < kSetCutBatch; j++)
  {
    const uint64_t r = r0 + j * 1024 + threadIdx.x;
    in[j] = r < n;
    g[j] = cp.ranges[in[j] ? r : 0];
  }
#pragma unroll
  for (uint32_t j = 0; j < kSetCutBatch; j++)
  {
    const uint32_t m = g[j].member < cp.n_members ? g[j].member : cp.n_members - 1;
    const GatherSetMember *rec = cp.members + m;
    segment[j] = rec->segment;
    decoded_len[j] = rec->decoded_len;
    out_lo[j] = rec->out_lo;
    out_hi[j] = rec->out_hi;
    pos[j] = cp.position[m];
  }
  bool ok = true;
#pragma unroll
  for (uint32_t j = 0; j < kSetCutBatch; j++)
  {
    bool good = g[j].member < cp.n_members && g[j].reserved == 0 &&
                gather_range_ok(g[j].offset, g[j].length, g[j].dst_offset, decoded_len[j], out_lo[j], out_hi[j], cp.dst_capacity);
    uint64_t t = 0;
    if (good && g[j].length != 0)
    {
      good = segment[j] != 0;
      t = good ? gather_range_tasks(g[j].offset, g[j].length, segment[j]) : 0;
      good = good && t < (1ull << 31);
    }
    tasks[j] = in[j] && good ? (uint32_t)t : 0;
    ok = ok && (good || !in[j]);
  }
  return ok;
}
// Rows of one member often stand together, and 64 lanes adding to one word are served one after the other: a wave adds once per key.
// The lanes that have `has` form groups by key: the lowest lane of a group is its leader (returned, for every lane of the group), `size`
// the group's lanes and `rank` the lanes of the group below this one.  No memory access in the loop: the leaders then add together.
__device__ __forceinline__ uint32_t set_cut_groups(uint32_t key, bool has, uint32_t &size, uint32_t &rank)
{
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long todo = __builtin_amdgcn_ballot_w64(has);
  uint32_t my_lead = lane;
  size = rank = 0;
  while (todo != 0)
  {
    const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)lead);
    const unsigned long long group = __builtin_amdgcn_ballot_w64(has && key == k);
    if (has && key == k)
    {
      my_lead = lead;
      size = (uint32_t)__popcll(group);
      rank = (uint32_t)__popcll(group & ((1ull << lane) - 1));
    }
    todo &= ~group;
  }
  return my_lead;
}
// counters[key] += the lanes that have `has` and this key
__device__ __forceinline__ void set_cut_count(uint32_t *counters, uint32_t key, bool has)
{
  uint32_t size, rank;
  const uint32_t lead = set_cut_groups(key, has, size, rank);
  if (has && lead == (threadIdx.x & 63))
    atomicAdd(counters + key, size);
}
// ... and the same with every lane's own place: counters[key] before the wave's add plus the lanes of its key below it (lanes without
// `has`: undefined)
__device__ __forceinline__ uint32_t set_cut_take(uint32_t *counters, uint32_t key, bool has)
{
  uint32_t size, rank, base = 0;
  const uint32_t lead = set_cut_groups(key, has, size, rank);
  if (has && lead == (threadIdx.x & 63))
    base = atomicAdd(counters + key, size);
  return (uint32_t)__shfl((int)base, (int)lead, 64) + rank;
}

// One workgroup of 1024 threads.  Steps, each behind a barrier: (1) the per-position counters are zeroed; (2) every range is checked, and
// those that have tasks are counted into their positions; (3) the counts are scanned into slot_first; (4) the ranges that have tasks are
// scattered into perm[], their task counts beside them; (5) those are scanned into first_task[]; (6) the tasks of every position of a
// shared kind — first_task at its slots' two ends — give its units, scanned into unit_first; then the kinds' totals are written.  One
// range that is refused, a count above max_count or a task total of 2^31 or more refuses the whole call: every total is written as 0
// and kStatusBadRange set in the set's word.  Every word a k_set_ranges launch reads is written by every call.
__global__ void __launch_bounds__(1024) k_set_cut(GatherSetCutParams cp)
{
  __shared__ uint64_t wave_sum[16];
  __shared__ uint32_t any_bad;
  const GatherSetWs ws = gather_set_ws(cp.n_members, cp.max_count);
  uint32_t *const hdr = cp.workspace, *const slot_first = cp.workspace + ws.slot_first, *const unit_first = cp.workspace + ws.unit_first;
  uint32_t *const cursor = cp.workspace + ws.cursor, *const perm = cp.workspace + ws.perm, *const first_task = cp.workspace + ws.first_task;
  const uint32_t M = cp.n_members;
  uint32_t n = cp.count != nullptr ? *cp.count : cp.max_count;
  bool bad = n > cp.max_count;
  if (bad)
    n = 0;
  if (threadIdx.x == 0)
    any_bad = 0;
  for (uint32_t p = threadIdx.x; p <= M; p += 1024)
  {
    set_ws_store(slot_first + p, 0);
    set_ws_store(cursor + p, 0);
  }
  set_cut_sync();

  // (2); what the first batch found stays in registers for (4): a call of up to 4096 rows reads them once
  uint32_t tasks0[kSetCutBatch] = {}, pos0[kSetCutBatch] = {};
  uint64_t mine = 0; // this thread's tasks
  for (uint64_t r0 = 0; r0 < n; r0 += 1024 * kSetCutBatch)
  {
    uint32_t tasks[kSetCutBatch], pos[kSetCutBatch];
    if (!set_cut_rows(cp, r0, n, tasks, pos))
      bad = true;
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      set_cut_count(slot_first, pos[j], tasks[j] != 0);
      mine += tasks[j];
      if (r0 == 0)
      {
        tasks0[j] = tasks[j];
        pos0[j] = pos[j];
      }
    }
  }
  uint64_t total = 0;
  (void)set_cut_scan(mine, wave_sum, total);
  if (bad || total >= (1ull << 31))
    any_bad = 1; // (benign race: every writer stores 1)
  set_cut_sync();
  if (any_bad != 0) // (the same on every thread)
  {
    if (threadIdx.x < kSetWsHeader)
      set_ws_store(hdr + threadIdx.x, 0);
    if (threadIdx.x == 0)
      atomicOr(cp.status, kStatusBadRange);
    return;
  }

  // (3) in place: a thread reads its own position's count, then overwrites it
  uint64_t slots = 0;
  for (uint32_t p0 = 0; p0 < M; p0 += 1024)
  {
    const uint32_t p = p0 + threadIdx.x;
    const uint32_t my_slots = p < M ? set_ws_load(slot_first + p) : 0;
    const uint64_t s = set_cut_scan(my_slots, wave_sum, slots);
    if (p < M)
      set_ws_store(slot_first + p, (uint32_t)s);
  }
  if (threadIdx.x == 0)
    set_ws_store(slot_first + M, (uint32_t)slots);
  set_cut_sync();

  // (4) in any order inside a position: the tasks tile the ranges whatever it is
  for (uint64_t r0 = 0; r0 < n; r0 += 1024 * kSetCutBatch)
  {
    uint32_t tasks[kSetCutBatch], pos[kSetCutBatch];
    if (r0 != 0)
      (void)set_cut_rows(cp, r0, n, tasks, pos);
    uint32_t first[kSetCutBatch];
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      if (r0 == 0)
      {
        tasks[j] = tasks0[j];
        pos[j] = pos0[j];
      }
      first[j] = set_ws_load(slot_first + pos[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      const uint64_t slot = (uint64_t)first[j] + set_cut_take(cursor, pos[j], tasks[j] != 0);
      if (tasks[j] != 0 && slot < slots) // (rows that were rewritten under the call must not reach outside the workspace)
      {
        set_ws_store(perm + slot, (uint32_t)(r0 + j * 1024 + threadIdx.x));
        set_ws_store(first_task + slot, tasks[j]);
      }
    }
  }
  set_cut_sync();

  // (5) in place
  uint64_t tasks_before = 0;
  for (uint64_t s0 = 0; s0 < slots; s0 += 1024 * kSetCutBatch)
  {
    uint32_t my_tasks[kSetCutBatch];
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      const uint64_t s = s0 + j * 1024 + threadIdx.x;
      my_tasks[j] = s < slots ? set_ws_load(first_task + s) : 0;
    }
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      const uint64_t s = s0 + j * 1024 + threadIdx.x;
      const uint64_t before = set_cut_scan(my_tasks[j], wave_sum, tasks_before);
      if (s < slots)
        set_ws_store(first_task + s, (uint32_t)before);
    }
  }
  if (threadIdx.x == 0)
    set_ws_store(first_task + slots, (uint32_t)tasks_before);
  set_cut_sync();

  // (6) the positions of the shared kinds are one run, [kind_first[3], M)
  uint64_t units = 0;
  if (threadIdx.x == 0)
    set_ws_store(unit_first + M, 0); // (where the set has no member of a shared kind)
  for (uint32_t p = threadIdx.x; p < cp.kind_first[3]; p += 1024)
    set_ws_store(unit_first + p, 0);
  for (uint32_t p0 = cp.kind_first[3]; p0 < M; p0 += 1024 * kSetCutBatch)
  {
    uint32_t lo[kSetCutBatch], hi[kSetCutBatch], t_lo[kSetCutBatch], t_hi[kSetCutBatch];
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      const uint32_t p = p0 + j * 1024 + threadIdx.x;
      lo[j] = p < M ? set_ws_load(slot_first + p) : 0;
      hi[j] = p < M ? set_ws_load(slot_first + p + 1) : 0;
    }
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      t_lo[j] = set_ws_load(first_task + lo[j]);
      t_hi[j] = set_ws_load(first_task + hi[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kSetCutBatch; j++)
    {
      const uint32_t p = p0 + j * 1024 + threadIdx.x;
      uint32_t my_units = 0;
      for (uint32_t k = 3; k < kGatherKinds; k++)
        if (p >= cp.kind_first[k] && p < cp.kind_first[k + 1])
          my_units = (t_hi[j] - t_lo[j] + cp.kind_waves[k] - 1) / cp.kind_waves[k];
      const uint64_t u = set_cut_scan(my_units, wave_sum, units);
      if (p < M)
        set_ws_store(unit_first + p, (uint32_t)u);
    }
    if (threadIdx.x == 0)
      set_ws_store(unit_first + M, (uint32_t)units);
  }
  set_cut_sync();
  if (threadIdx.x < kSetWsHeader)
  {
    const uint32_t k = threadIdx.x - kSetWsTasks, ku = threadIdx.x - kSetWsUnits, ks = threadIdx.x - kSetWsSlot;
    uint32_t v = 0;
    if (k < kGatherKinds)
      v = set_ws_load(first_task + set_ws_load(slot_first + cp.kind_first[k + 1])) - set_ws_load(first_task + set_ws_load(slot_first + cp.kind_first[k]));
    else if (ku >= 3 && ku < kGatherKinds)
      v = set_ws_load(unit_first + cp.kind_first[ku + 1]) - set_ws_load(unit_first + cp.kind_first[ku]);
    else if (ks <= kGatherKinds)
      v = set_ws_load(slot_first + cp.kind_first[ks]);
    else if (threadIdx.x == kSetWsCount)
      v = n;
    set_ws_store(hdr + threadIdx.x, v);
  }
}

// the last i in [lo, hi) with a[i] <= t (a ascending, a[lo] <= t; all wave-uniform)
__device__ __forceinline__ uint32_t set_search(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t t)
{
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (uni(a[mid]) <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// task `task` (counted over all kinds) of the range in perm slot `slot`: the range cut at the absolute multiples of its member's segment
template <int MODE, bool SHARED>
__device__ __forceinline__ void set_run_task(WaveCtx &c, const PlanView &pv, const GatherSetRangesParams &rp, const GatherSetRange *g, uint64_t segment, uint32_t nth)
{
  const uint64_t offset = uni64(g->offset), stop = offset + uni64(g->length), dst_offset = uni64(g->dst_offset);
  const uint64_t cut = (uni64(offset / segment) + nth) * segment;
  const uint64_t begin = cut > offset ? cut : offset, end = cut + segment < stop ? cut + segment : stop;
  run_gather<MODE, SHARED>(c, pv, rp.dst, begin, end, (int64_t)(dst_offset - offset));
}
// the stream of a member's record (all wave-uniform); SHARED: with its host-built table
template <bool SHARED>
__device__ __forceinline__ GatherSource set_source(const GatherSetMember *rec, bool check_hist)
{
  GatherSource gs{};
  gs.stream = (const uint8_t *)uni64((uint64_t)(uintptr_t)rec->src.stream);
  gs.stream_len = uni64(rec->src.stream_len);
  gs.plan = (const uint8_t *)uni64((uint64_t)(uintptr_t)rec->src.plan);
  gs.status = (uint32_t *)uni64((uint64_t)(uintptr_t)rec->src.status);
  if (SHARED)
    gs.table = (const uint2 *)uni64((uint64_t)(uintptr_t)rec->src.table);
  if (check_hist)
  {
    gs.hist_copy = (const uint16_t *)uni64((uint64_t)(uintptr_t)rec->src.hist_copy);
    gs.hist_off = uni64(rec->src.hist_off);
  }
  return gs;
}

// blockDim.x = 64 * waves, any grid; LDS as k_gather_set.
// A table per wave (kinds 0..2): waves stride over the kind's tasks as k_gather_ranges' do; a wave finds its task's perm slot by binary
// search in first_task, takes the range, then its member's record, and runs the task.
// One table per workgroup (kinds 3..5): workgroup b serves the kind's units [b * per, (b + 1) * per), per = ceil(units / gridDim.x); a unit
// is `waves` consecutive tasks of one member, found by binary search in unit_first; the member's table is copied where the member differs
// from that of the workgroup's unit before, and the workgroup that serves a member's first unit checks its histogram.  Every loop bound is
// the same for the whole workgroup: all its waves reach every barrier.
template <int MODE, bool SHARED>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(100))) k_set_ranges(GatherSetRangesParams rp)
{
  extern __shared__ u32x4 smem_v[];
  const GatherSetWs ws = gather_set_ws(rp.n_members, rp.max_count);
  const uint32_t *const slot_first = rp.workspace + ws.slot_first, *const unit_first = rp.workspace + ws.unit_first;
  const uint32_t *const perm = rp.workspace + ws.perm, *const first_task = rp.workspace + ws.first_task;
  const uint32_t waves = blockDim.x >> 6, wave = uni(threadIdx.x >> 6);
  WaveCtx c;
  if (!SHARED)
  {
    const uint32_t total = uni(rp.workspace[kSetWsTasks + rp.kind]);
    if (blockIdx.x >= total)
      return;
    const uint32_t s_lo = uni(rp.workspace[kSetWsSlot + rp.kind]), s_hi = uni(rp.workspace[kSetWsSlot + rp.kind + 1]);
    const uint32_t t0 = uni(first_task[s_lo]);
    const uint32_t stride = gridDim.x * waves;
    for (uint32_t t = wave * gridDim.x + blockIdx.x; t < total; t += stride)
    {
      const uint32_t slot = set_search(first_task, s_lo, s_hi, t0 + t);
      const GatherSetRange *g = rp.ranges + uni(perm[slot]);
      const GatherSetMember *rec = rp.members + uni(g->member);
      const GatherSource gs = set_source<false>(rec, false);
      gather_setup<MODE, false>(c, gs, uni(rec->bits), uni(rec->states), wave, rp.table_bytes, false, (uint8_t *)smem_v);
      set_run_task<MODE, false>(c, plan_view(gs.plan), rp, g, uni64(rec->segment), t0 + t - uni(first_task[slot]));
    }
  }
  else
  {
    const uint32_t units = uni(rp.workspace[kSetWsUnits + rp.kind]);
    const uint32_t per = units > gridDim.x ? (units + gridDim.x - 1) / gridDim.x : 1;
    const uint64_t u_lo = (uint64_t)blockIdx.x * per;
    if (u_lo >= units)
      return;
    const uint32_t u_hi = u_lo + per < units ? (uint32_t)(u_lo + per) : units;
    const uint32_t u0 = uni(unit_first[rp.pos_lo]);
    uint32_t have = 0xFFFFFFFFu; // the position whose table the LDS holds
    const GatherSetMember *rec = nullptr;
    PlanView pv{};
    uint32_t s_lo = 0, s_hi = 0, t_lo = 0, t_hi = 0, u_first = 0;
    for (uint32_t u = (uint32_t)u_lo; u < u_hi; u++)
    {
      const uint32_t p = set_search(unit_first, rp.pos_lo, rp.pos_hi, u0 + u);
      if (p != have)
      {
        if (have != 0xFFFFFFFFu)
          __syncthreads(); // (every wave is done with the table that is about to be overwritten)
        have = p;
        s_lo = uni(slot_first[p]);
        s_hi = uni(slot_first[p + 1]);
        t_lo = uni(first_task[s_lo]);
        t_hi = uni(first_task[s_hi]);
        u_first = uni(unit_first[p]);
        rec = rp.members + uni(rp.ranges[uni(perm[s_lo])].member); // (a position that has units has a range)
        const bool check_hist = u0 + u == u_first && threadIdx.x < 64;
        const GatherSource gs = set_source<true>(rec, check_hist);
        pv = plan_view(gs.plan);
        gather_setup<MODE, true>(c, gs, uni(rec->bits), uni(rec->states), wave, rp.table_bytes, check_hist, (uint8_t *)smem_v);
      }
      const uint32_t t = t_lo + (u0 + u - u_first) * waves + wave;
      if (t < t_hi)
      {
        const uint32_t slot = set_search(first_task, s_lo, s_hi, t);
        set_run_task<MODE, true>(c, pv, rp, rp.ranges + uni(perm[slot]), uni64(rec->segment), t - uni(first_task[slot]));
      }
    }
  }
}

} // namespace hsrans

#endif // HSRANS_KERNELS_GATHER_H
