// kernels_walk.h — K2: the mt_ header chain followed on the device — k_mt_chase, k_mt_fill; the indexed plan assembled behind a first decode — k_index_count, k_index_fill (mt_), k_walk_index_count, k_walk_index_fill (block_).
// Part of the one device translation unit hsrans_kernels.hip (which includes the parts in dependency order and holds the host-side launcher).
#ifndef HSRANS_KERNELS_WALK_H
#define HSRANS_KERNELS_WALK_H

namespace hsrans
{

// ---------------------------------------------------------------------------------------------------------------
// K2: mt_ header-chain walk on the device (one wavefront; lane 0 steers, all lanes copy states / sum counts).
// Mirrors hsrans::plan_build's mt_ branch step by step, which mirrors mt_rANS32x64_16w_decode.cpp:41-96.
// plan == nullptr: count only.  Otherwise plan is a blob sized for `n_chains` single-piece chains: the kernel fills
// chain_first, pieces and states (the host writes the 64-byte header).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t load_u64_2b(const uint8_t *p) // stream offsets are only 2-byte aligned
{
  uint64_t v = 0;
  for (int b = 3; b >= 0; b--)
    v = (v << 16) | *(const uint16_t *)(p + 2 * b);
  return v;
}

// Pass 1, the pointer chase (one wavefront, all lanes in lockstep on uniform values): per block ONE 16-byte read
// {size, skip}, nothing else — the next header's position depends on it, so this read is the whole critical path.  Every
// block's {header position, output offset} goes to `blocks`; everything that is not needed to find the next header (start
// states, histogram sum check, the piece records) is left to pass 2, which is parallel over the blocks.
__global__ void __launch_bounds__(64) k_mt_chase(const uint8_t *in, uint64_t in_len, uint64_t out_cap, uint32_t S, uint64_t *blocks, uint32_t max_blocks,
                                                 WalkResult *result)
{
  uint32_t count = 0, error = 0;
  uint64_t out_len = 0;
  do
  {
    // the checks every reference decoder opens with (mt_…decode.cpp:15-32)
    if (in_len < 16 + 4 * (uint64_t)S + 512) { error = 1; break; }
    out_len = uni64(load_u64_2b(in));
    const uint64_t stored = uni64(load_u64_2b(in + 8));
    if (out_len > out_cap || in_len < stored || out_len == 0 || out_len + 1 < S) { error = 1; break; }
    const uint64_t whole = out_len - S + 1;
    uint64_t pos = 16, i = 0;
    bool last_is_rans = false;
    do
    {
      if (pos + 8 > in_len) { error = 2; break; }
      const uint64_t at = pos;
      // {size, skip} in one go; the skip word only exists (and is only used) for coded blocks, so it is read only when in range
      const bool have16 = pos + 16 <= in_len;
      uint64_t size_val = load_u64_2b(in + pos);
      uint64_t skip = have16 ? load_u64_2b(in + pos + 8) : 0;
      size_val = uni64(size_val);
      skip = uni64(skip);
      pos += 8;
      const uint64_t i0 = i;
      if (size_val >> 63)
      {
        const uint64_t len = size_val & (((uint64_t)1 << 54) - 1);
        if (len == 0 || i > out_len || len > out_len - i) { error = 3; break; }
        i += len;
        last_is_rans = false;
      }
      else
      {
        if (pos + 8 + 4 * (uint64_t)S + 512 > in_len) { error = 2; break; }
        pos += 8;
        if (skip > in_len) { error = 2; break; }
        const uint64_t after = pos + 2 * (skip + 1);
        uint64_t end = i + size_val;
        if (end > whole || end < i)
          end = whole;
        else if (end & (S - 1)) { error = 5; break; }
        const uint64_t steps = end > i ? (end - i + S - 1) / S : 0;
        if (steps > 0xFFFFFFFFull || size_val == 0) { error = 5; break; }
        i += steps * S;
        last_is_rans = true;
        pos = i > whole ? ~(uint64_t)0 : after; // both outcomes of mt_…decode.cpp:86-92 leave the loop
      }
      if (i >= whole && i < out_len && (!last_is_rans || out_len - i >= S)) { error = 6; break; } // see hsrans::plan_build
      if (count >= max_blocks) { error = 7; break; } // the block list is full: the host retries with a larger one
      if (threadIdx.x == 0)
      {
        blocks[2 * (uint64_t)count] = at;
        blocks[2 * (uint64_t)count + 1] = i0;
      }
      count++;
      if (pos == ~(uint64_t)0)
        break;
    } while (i < whole);
  } while (false);
  if (threadIdx.x == 0)
  {
    result->n_chains = count;
    result->error = error;
    result->decoded_len = out_len;
  }
}

// Pass 2, one wavefront per block: the block's chain record, start states and histogram sum check (what
// mt_…decode.cpp:62-72 reads from a block header), written into the plan blob sized for n_chains chains.
__global__ void __launch_bounds__(64) k_mt_fill(const uint8_t *in, uint64_t in_len, uint32_t S, uint32_t bits, const uint64_t *blocks, uint8_t *plan,
                                                uint32_t n_chains, uint64_t out_len, WalkResult *result)
{
  const uint32_t b = blockIdx.x, lane = threadIdx.x;
  uint32_t *cf = (uint32_t *)(plan + plan_chain_first_off());
  Piece *pieces = (Piece *)(plan + plan_pieces_off(n_chains));
  uint32_t *states = (uint32_t *)(plan + plan_states_off(n_chains, n_chains));
  const uint64_t whole = out_len - S + 1;
  uint64_t pos = blocks[2 * (uint64_t)b];
  const uint64_t i = blocks[2 * (uint64_t)b + 1];
  const uint64_t size_val = uni64(load_u64_2b(in + pos));
  pos += 8;
  Piece p{};
  uint64_t i_end = i;
  if (size_val >> 63)
  {
    p.flags = kPieceFill | kPieceChainStart;
    p.out_off = i;
    p.fill_len = size_val & (((uint64_t)1 << 54) - 1);
    p.hist_off = (size_val >> 54) & 0xFF;
    i_end = i + p.fill_len;
  }
  else
  {
    pos += 8; // skip
    if (lane < S)
      states[(uint64_t)b * S + lane] = (uint32_t)*(const uint16_t *)(in + pos + 4 * lane) | ((uint32_t)*(const uint16_t *)(in + pos + 4 * lane + 2) << 16);
    pos += 4 * (uint64_t)S;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < 4; k++)
      sum += *(const uint16_t *)(in + pos + 2 * (4 * lane + k));
    for (int d = 32; d >= 1; d >>= 1)
      sum += __shfl_xor(sum, d, 64);
    if (uni(sum) != (1u << bits) && lane == 0) // inplace_complete_hist, hist.cpp:308-324
      atomicMax(&result->error, 4u);
    p.flags = kPieceChainStart;
    p.hist_off = pos;
    p.words_off = pos + 512;
    p.out_off = i;
    uint64_t end = i + size_val;
    if (end > whole || end < i)
      end = whole;
    const uint64_t steps = end > i ? (end - i + S - 1) / S : 0;
    p.steps = (uint32_t)steps;
    i_end = i + steps * S;
  }
  p.state_idx = b;
  if (i_end >= whole && i_end < out_len)
    p.tail = (uint16_t)(out_len - i_end); // final partial group: a tail on the last chain (mt_…decode.cpp:99-130)
  if (lane == 0)
  {
    pieces[b] = p;
    cf[b] = b;
    if (b + 1 == n_chains)
      cf[n_chains] = n_chains;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The indexed plan of a stream whose first decode has just recorded its checkpoints (hsrans_decode_device_indexing), assembled
// ON THE DEVICE: the base plan (one single-piece chain per mt_ block), the states and read cursors the recording pass left every
// `interval` groups (slot = absolute group / interval) -> the plan with one chain per block start and per checkpoint inside the
// blocks, plus the Group records of the grouped launch.  The chains of a block are the host's own rule (IndexBlock, hsrans_kernels.h).
// (Round 3 brought 7.5-15 MB of checkpoints down to the host, assembled the blob on one core and sent it up again: 0.8 ms of the
// first decode's 1.3-2.5 ms.)
//   k_index_count   one workgroup: chains per block, their exclusive scan -> chain_off[], the totals and header facts -> *result
//   k_index_fill    one wavefront per block: header, chain table, pieces, start states, groups
// ---------------------------------------------------------------------------------------------------------------
// One value per thread of a 1024-thread workgroup -> its exclusive prefix, continued from call to call through *carry (LDS: zeroed by the
// caller, one barrier before the first call; the running total afterwards).  Every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t wg_scan_1024(uint32_t v, uint32_t *wave_tot, uint32_t *carry)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o = __shfl_up(incl, d, 64);
    if ((int)lane >= d)
      incl += o;
  }
  if (lane == 63)
    wave_tot[wave] = incl;
  __syncthreads();
  uint32_t before = *carry;
  for (uint32_t w = 0; w < wave; w++)
    before += wave_tot[w];
  __syncthreads();
  if (threadIdx.x == 1023)
    *carry = before + incl;
  __syncthreads();
  return before + incl - v;
}

// what one wavefront writes for a block both ways: the new plan's header (the base plan's container, states, bits and lengths), ...
__device__ __forceinline__ void index_write_header(const uint8_t *base, uint8_t *plan, const IndexResult &r, uint32_t interval)
{
  const PlanHeader &hb = *(const PlanHeader *)base;
  PlanHeader h{}; // (flags: none)
  for (int i = 0; i < 8; i++)
    h.magic[i] = hb.magic[i];
  h.container = hb.container;
  h.states = hb.states;
  h.bits = hb.bits;
  h.decoded_len = hb.decoded_len;
  h.stream_len = hb.stream_len;
  h.n_chains = h.n_pieces = r.chains;
  h.interval = interval;
  h.shared_hist = r.coded == 1 ? 1 : 0; // (plans K2 wrote leave these two clear even for a single block)
  h.aux_off = h.shared_hist ? r.hist_off : 0;
  *(PlanHeader *)plan = h;
  ((uint32_t *)(plan + plan_chain_first_off()))[r.chains] = r.chains;
}
// ... and the block's `count` chains from chain c0 on: chain table, pieces, start states (entry: those the block is entered with)
__device__ __forceinline__ void index_write_chains(const IndexBlock &blk, uint32_t S, uint32_t interval, uint32_t c0, uint32_t count, const uint32_t *entry,
                                                   const uint32_t *ck_states, const uint64_t *ck_words, uint8_t *plan, uint32_t nc)
{
  const uint32_t lane = threadIdx.x;
  uint32_t *chain_first = (uint32_t *)(plan + plan_chain_first_off());
  Piece *pieces = (Piece *)(plan + plan_pieces_off(nc));
  uint32_t *states = (uint32_t *)(plan + plan_states_off(nc, nc));
  for (uint32_t k = lane; k < count; k += 64)
  {
    pieces[c0 + k] = index_chain_piece(blk, S, interval, k, ck_words, c0 + k);
    chain_first[c0 + k] = c0 + k;
  }
  for (uint32_t k = 0; k < count; k++)
    if (lane < S)
    {
      const uint32_t *st = index_chain_states(blk, S, interval, k, entry, ck_states);
      states[(uint64_t)(c0 + k) * S + lane] = st ? st[lane] : 0;
    }
}
// chains [begin, begin + count) as a group
__device__ __forceinline__ Group index_group(uint32_t begin, uint32_t count, uint32_t flags, uint64_t hist_off, uint64_t words_end)
{
  return Group{begin, count, flags, begin, hist_off, words_end};
}
// part `part` of `parts` of a coded block's chains as a group
__device__ __forceinline__ Group index_part_group(const IndexBlock &blk, uint32_t interval, uint32_t c0, uint32_t count, uint32_t part, uint32_t parts,
                                                  const uint64_t *ck_words, uint64_t words_end)
{
  const IndexPart r = index_block_part(blk, interval, count, part, parts, ck_words, words_end);
  return index_group(c0 + r.lo, r.hi - r.lo, kGroupMergeable, blk.hist_off, r.words_end);
}

// (the four bodies are device functions of their argument struct: the kernels below hand them their own, by value in the kernel arguments; the
// batch forms of kernels_index_batch.h hand them member m's, from a table in device memory)
// groups block ch of an mt_ base plan opens before any is cut: a coded block one, a run of single-symbol blocks one at its first block
__device__ __forceinline__ uint32_t index_block_leads(const uint32_t *cf0, const Piece *pc0, uint32_t ch, bool fill)
{
  return !fill || ch == 0 || !(pc0[cf0[ch - 1]].flags & kPieceFill) ? 1 : 0;
}

// chains and groups per block, their exclusive scans, the totals and header facts -> *result.  The group list is the one dplan_fill derives
// from the finished blob: one group per coded block, cut into group_parts_of parts where there are few, one per run of single-symbol blocks,
// packed; none where there would be as many groups as chains
__device__ __forceinline__ void index_count(const IndexArgs &a)
{
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t carry_s, coded_s, first_s, last_s, fewest_s, lead_s;
  __shared__ unsigned long long hist_s;
  const uint32_t *cf0 = (const uint32_t *)(a.base + plan_chain_first_off());
  const Piece *pc0 = (const Piece *)(a.base + plan_pieces_off(a.n_base));
  if (threadIdx.x == 0)
  {
    carry_s = coded_s = last_s = lead_s = 0;
    first_s = 0xFFFFFFFFu;
    fewest_s = kIndexNoFewest;
    hist_s = 0;
  }
  __syncthreads();
  for (uint32_t base = 0; base < a.n_base; base += 1024)
  {
    const uint32_t ch = base + threadIdx.x;
    uint32_t v = 0;
    if (ch < a.n_base)
    {
      const IndexBlock blk = index_block_of_piece(pc0[cf0[ch]], a.S, ch + 1 == a.n_base);
      v = index_block_chains(blk, a.interval);
      atomicAdd(&lead_s, index_block_leads(cf0, pc0, ch, blk.fill));
      if (!blk.fill) // (mt_ blocks never share a histogram)
      {
        atomicAdd(&coded_s, 1u);
        atomicMin(&first_s, ch);
        atomicMax(&last_s, ch);
        atomicMax(&hist_s, (unsigned long long)blk.hist_off);
      }
    }
    const uint32_t off = wg_scan_1024(v, wave_tot, &carry_s);
    if (ch < a.n_base)
      a.chain_off[ch] = off;
  }
  const uint32_t total = carry_s, lead = lead_s;
  // dplan_fill: groups only where there are fewer than chains, cut into parts where there are few
  const bool grouped = lead < total;
  const uint32_t k_max = grouped ? group_parts_max_of(a.parts_want, lead) : 1;
  __syncthreads();
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < a.n_base; base += 1024)
  {
    const uint32_t ch = base + threadIdx.x;
    uint32_t v = 0;
    if (ch < a.n_base)
    {
      const IndexBlock blk = index_block_of_piece(pc0[cf0[ch]], a.S, ch + 1 == a.n_base);
      const uint32_t count = index_block_chains(blk, a.interval);
      v = blk.fill ? index_block_leads(cf0, pc0, ch, true) : group_parts_of(count, k_max);
      if (!blk.fill && ch != first_s && ch != last_s)
        atomicMin(&fewest_s, count);
    }
    const uint32_t off = wg_scan_1024(v, wave_tot, &carry_s);
    if (ch < a.n_base)
      a.group_off[ch] = off;
  }
  if (threadIdx.x == 0)
  {
    const uint32_t n_groups = carry_s;
    IndexResult r{};
    r.chains = total;
    r.blocks = a.n_base;
    r.coded = coded_s;
    r.fewest = fewest_s;
    r.hist_off = hist_s;
    r.groups = grouped ? n_groups : 0; // (as many groups as chains — no checkpoint fell inside any block: the ungrouped launch)
    r.parts = k_max;
    r.error = total > a.max_chains || n_groups > a.max_groups ? 3 : 0;
    *a.result = r;
  }
}

__global__ void __launch_bounds__(1024) k_index_count(IndexArgs a) { index_count(a); }

// block (base chain) `ch` of the plan, by one wavefront
__device__ __forceinline__ void index_fill(const IndexArgs &a, uint32_t ch)
{
  const uint32_t lane = threadIdx.x, S = a.S;
  const IndexResult r = *a.result;
  if (r.error != 0) // (more chains or groups than the host sized the arena for: it reads the result and fails the call)
    return;
  const uint32_t *cf0 = (const uint32_t *)(a.base + plan_chain_first_off());
  const Piece *pc0 = (const Piece *)(a.base + plan_pieces_off(a.n_base));
  const uint32_t *st0 = (const uint32_t *)(a.base + plan_states_off(a.n_base, a.n_base));
  const Piece bp = pc0[cf0[ch]];
  const IndexBlock blk = index_block_of_piece(bp, S, ch + 1 == a.n_base);
  const uint32_t c0 = a.chain_off[ch], count = index_block_chains(blk, a.interval);
  if (ch == 0 && lane == 0)
    index_write_header(a.base, a.plan, r, a.interval);
  index_write_chains(blk, S, a.interval, c0, count, st0 + (uint64_t)bp.state_idx * S, a.ck_states, a.ck_words, a.plan, r.chains);
  if (a.groups == nullptr || r.groups == 0 || !index_block_leads(cf0, pc0, ch, blk.fill))
    return;
  // the group's words end at the next rANS block's histogram (as dplan_fill has it), or at the stream's end
  uint64_t words_end = a.stream_len;
  uint32_t run = 1; // a single-symbol block: the blocks of its run
  for (uint32_t nx = ch + 1; nx < a.n_base; nx++)
  {
    const Piece &q = pc0[cf0[nx]];
    if (!(q.flags & kPieceFill))
    {
      words_end = q.hist_off;
      break;
    }
    run++; // (every block passed here is a single-symbol one: behind a run's first block, the rest of its run)
  }
  const uint32_t g0 = a.group_off[ch];
  if (blk.fill)
  {
    if (lane == 0)
      a.groups[g0] = index_group(c0, run, kGroupFill, 0, words_end);
    return;
  }
  const uint32_t parts = group_parts_of(count, r.parts);
  for (uint32_t part = lane; part < parts; part += 64)
    a.groups[g0 + part] = index_part_group(blk, a.interval, c0, count, part, parts, a.ck_words, words_end);
}

__global__ void __launch_bounds__(64) k_index_fill(IndexArgs a) { index_fill(a, blockIdx.x); }

// ---------------------------------------------------------------------------------------------------------------
// The same for a block_ stream, from the records of the walk that has just decoded it (run_block_walk with ckpt_interval != 0): the plan
// hsrans_index_build(HSRANS_BLOCK) returns and the group list dplan_fill derives from that plan — one group per coded block, cut into
// parts where there are few (group_parts_of), one per run of single-symbol blocks.  The block count is read here, not on the host: the
// grids are sized by the host's bound.
//   k_walk_index_count   one workgroup: chains and groups per block, their exclusive scans, the totals and header facts -> *result
//   k_walk_index_fill    one wavefront per block (striding): header, chain table, pieces, start states, groups
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ IndexBlock walk_index_block(const WalkIndexArgs &a, uint32_t b, uint32_t n)
{
  return index_block_of_walk(a.walk_blocks[3 * (uint64_t)b], a.walk_blocks[3 * (uint64_t)b + 1], a.walk_blocks[3 * (uint64_t)b + 2], a.decoded_len, a.S, b + 1 == n);
}
// groups block b opens before any is cut: a coded block one, a run of single-symbol blocks one at its first block
__device__ __forceinline__ uint32_t walk_block_leads(const WalkIndexArgs &a, uint32_t b, bool fill)
{
  return !fill || b == 0 || !(a.walk_blocks[3 * (uint64_t)(b - 1) + 2] >> 63) ? 1 : 0;
}

__device__ __forceinline__ void walk_index_count(const WalkIndexArgs &a)
{
  __shared__ uint32_t wave_tot[16];
  __shared__ uint32_t carry_s, coded_s, first_s, last_s, fewest_s, bad_s, lead_s;
  __shared__ unsigned long long hist_s;
  const uint32_t n = a.walk_count[0];
  if (n == 0 || n > a.max_blocks) // (uniform: the walk recorded nothing, or more blocks than the list holds)
  {
    if (threadIdx.x == 0)
      a.result->error = 1;
    return;
  }
  if (threadIdx.x == 0)
  {
    carry_s = coded_s = last_s = bad_s = lead_s = 0;
    first_s = 0xFFFFFFFFu;
    fewest_s = kIndexNoFewest;
    hist_s = 0;
  }
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 1024)
  {
    const uint32_t b = base + threadIdx.x;
    uint32_t v = 0;
    if (b < n)
    {
      const IndexBlock blk = walk_index_block(a, b, n);
      v = index_block_chains(blk, a.interval);
      atomicAdd(&lead_s, walk_block_leads(a, b, blk.fill));
      if (index_block_ends_short(blk, a.decoded_len))
        bad_s = 2;
      if (!blk.fill)
      {
        atomicAdd(&coded_s, 1u);
        atomicMin(&first_s, b);
        atomicMax(&last_s, b);
        atomicMax(&hist_s, (unsigned long long)blk.hist_off);
      }
    }
    const uint32_t off = wg_scan_1024(v, wave_tot, &carry_s);
    if (b < n)
      a.chain_off[b] = off;
  }
  const uint32_t total = carry_s, lead = lead_s;
  // dplan_fill: groups only where there are fewer than chains, cut into parts where there are few
  const bool grouped = lead < total;
  const uint32_t k_max = grouped ? group_parts_max_of(a.parts_want, lead) : 1;
  __syncthreads();
  if (threadIdx.x == 0)
    carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 1024)
  {
    const uint32_t b = base + threadIdx.x;
    uint32_t v = 0;
    if (b < n)
    {
      const IndexBlock blk = walk_index_block(a, b, n);
      const uint32_t count = index_block_chains(blk, a.interval);
      v = blk.fill ? walk_block_leads(a, b, true) : group_parts_of(count, k_max);
      if (!blk.fill && b != first_s && b != last_s)
        atomicMin(&fewest_s, count);
    }
    const uint32_t off = wg_scan_1024(v, wave_tot, &carry_s);
    if (b < n)
      a.group_off[b] = off;
  }
  if (threadIdx.x == 0)
  {
    const uint32_t n_groups = carry_s;
    IndexResult r{};
    r.chains = total;
    r.blocks = n;
    r.coded = coded_s;
    r.fewest = fewest_s;
    r.hist_off = hist_s;
    r.groups = grouped ? n_groups : 0;
    r.parts = k_max;
    r.error = bad_s ? bad_s : total > a.max_chains || n_groups > a.max_groups ? 3 : 0;
    *a.result = r;
  }
}

__global__ void __launch_bounds__(1024) k_walk_index_count(WalkIndexArgs a) { walk_index_count(a); }

// the wavefronts first, first + stride, ... of `stride` stride over the blocks
__device__ __forceinline__ void walk_index_fill(const WalkIndexArgs &a, uint32_t first, uint32_t stride)
{
  const IndexResult r = *a.result;
  if (r.error != 0) // no plan: the host reads the word and fails the call
    return;
  const uint32_t lane = threadIdx.x, S = a.S, n = r.blocks;
  if (first == 0 && lane == 0)
    index_write_header(a.base, a.plan, r, a.interval);
  for (uint32_t b = first; b < n; b += stride)
  {
    const IndexBlock blk = walk_index_block(a, b, n);
    const uint32_t c0 = a.chain_off[b], count = index_block_chains(blk, a.interval);
    index_write_chains(blk, S, a.interval, c0, count, a.walk_states + (uint64_t)b * S, a.ck_states, a.ck_words, a.plan, r.chains);
    if (r.groups == 0 || !walk_block_leads(a, b, blk.fill))
      continue;
    // the group's words end where the next coded block's histogram begins (as dplan_fill has it), or at the stream's end
    uint64_t words_end = a.stream_len;
    uint32_t run = 1; // a single-symbol block: the blocks of its run
    for (uint32_t nx = b + 1; nx < n; nx++)
    {
      if (!(a.walk_blocks[3 * (uint64_t)nx + 2] >> 63))
      {
        words_end = a.walk_blocks[3 * (uint64_t)nx] + 8;
        break;
      }
      run++; // (every block passed here is a single-symbol one: behind a run's first block, the rest of its run)
    }
    const uint32_t g0 = a.group_off[b];
    if (blk.fill)
    {
      if (lane == 0)
        a.groups[g0] = index_group(c0, run, kGroupFill, 0, words_end);
      continue;
    }
    const uint32_t parts = group_parts_of(count, r.parts);
    for (uint32_t part = lane; part < parts; part += 64)
      a.groups[g0 + part] = index_part_group(blk, a.interval, c0, count, part, parts, a.ck_words, words_end);
  }
}

__global__ void __launch_bounds__(64) k_walk_index_fill(WalkIndexArgs a) { walk_index_fill(a, blockIdx.x, gridDim.x); }

// ---------------------------------------------------------------------------------------------------------------
// 64-bit fingerprint of a stream in device memory (hsrans_decode_host's index cache: the index a first decode left behind may only
// serve a later call when EVERY byte of the stream is the same).  Fixed launch shape (the value depends on which thread reads which
// word): thread t folds the 16-byte words t, t + T, t + 2T, ... in order; the per-thread values are mixed with t and summed.
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kChecksumGrid = 1024, kChecksumBlock = 256;
__global__ void __launch_bounds__(kChecksumBlock) k_stream_checksum(const uint8_t *in, uint64_t n, unsigned long long *sum)
{
  const uint64_t T = (uint64_t)kChecksumGrid * kChecksumBlock, t = (uint64_t)blockIdx.x * kChecksumBlock + threadIdx.x;
  uint64_t h = 0x9E3779B97F4A7C15ull * (t + 1);
  const uint64_t words = n / 16;
  for (uint64_t i = t; i < words; i += T)
  {
    const uint4 w = ((const uint4 *)in)[i];
    h = (h ^ ((uint64_t)w.x | ((uint64_t)w.y << 32))) * 0xFF51AFD7ED558CCDull;
    h = (h ^ (h >> 29) ^ ((uint64_t)w.z | ((uint64_t)w.w << 32))) * 0xC4CEB9FE1A85EC53ull;
  }
  if (t == 0)
    for (uint64_t i = words * 16; i < n; i++)
      h = (h ^ in[i]) * 0xFF51AFD7ED558CCDull;
  h ^= h >> 32;
  // wave sum first: 4,096 atomics instead of 262,144
  for (int d = 32; d >= 1; d >>= 1)
    h += __shfl_xor(h, d, 64);
  if ((threadIdx.x & 63) == 0)
    atomicAdd(sum, (unsigned long long)h);
}

} // namespace hsrans

#endif // HSRANS_KERNELS_WALK_H
