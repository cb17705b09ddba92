// Launch interface between the C ABI (hsrans_capi.cpp) and the gfx950 kernels (hsrans_kernels.hip): the kernels' parameter structs and the
// launch_* functions.  What decides a launch — shapes, the kernel choice, shares — is hsrans_launch.h (hsrans_launch.cpp), included here.
#ifndef HSRANS_KERNELS_H
#define HSRANS_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hsrans_plan.h"
#include "hsrans_tuning.h"
#include "hsrans_launch.h"

namespace hsrans
{

// Persistent launch of a kPlanMergeable plan: everything a wave needs without a dependent read of the plan header.
// Chain c (local index) covers groups [c*interval, min((c+1)*interval, steps_total)) of the run that starts at out_base.
struct PersistentArgs
{
  const Piece *pieces;   // null = not a persistent launch
  const uint32_t *states;
  uint32_t n_chains, interval, S, bits; // interval == 0: chains of any length, one per wave (run_direct); else uniform chains

  uint64_t out_base, steps_total, hist_off;
  uint32_t tail;            // symbols of the final partial group (after the last chain)
  uint32_t static_per_wave; // chains every wave decodes as one merged run before it starts pulling single chains (mean)
  // 64-state launches: the static run of a wave depends on its slot, class k = (workgroup in the grid's second half) * 4
  // + (wave in workgroup / 4): the SIMD arbiter serves its oldest wave first, so equal shares finish far apart
  // (run_persistent).  run_len[k] chains; wave j of class k in workgroup b' of its half starts at
  // half_base[h] + b' * wg_chains[h] + class_off[k] + (j & 3) * run_len[k].  static_total = all static chains.
  uint32_t run_len[8], class_off[8], wg_chains[2], half_base[2], static_total;
  const uint2 *table;       // host-built decode table (kPlanHasHist plans) or null: build it in the kernel
  uint32_t table_mode;      // 3: one uint2 per slot; 4: the rank table (bits 13..15); 5: as 3, left in global memory; see kMode* in kernels_layout.h
  uint32_t dual;            // two chains per wave: k_decode_dual
  const uint16_t *hist_copy; // the 256 counts that table was built from (device copy inside the plan)
  unsigned long long *counters; // [kDynQueues * kDynQueueStride] monotonic queue heads of THIS launch's counter set (never reset, see run_persistent)
  // one-chain-per-wave launches (interval == 0, 64 states): the plan's chains are dealt to the launch's waves as runs of run_chains
  // consecutive chains, each decoded as one chain (run_direct; 1 for the index hsrans_index_boundaries makes for this device)
  uint32_t run_chains;
};
constexpr uint32_t kDynQueues = 64;
constexpr uint32_t kDynQueueStride = 32; // in uint64: one head per 256 B, so that heads never share a line / atomic unit
// A device plan owns kCounterSets sets of queue heads and every launch takes the next one (round robin): launches of one
// plan may overlap (several streams, double-buffered outputs), up to kCounterSets of them in flight at once (include/hsrans_hip.h).
constexpr uint32_t kCounterSets = 32;

// Grouped launch (block_/mt_ plans with checkpoints): chains [begin, begin+count) share one histogram = one LDS table
// per workgroup; its waves split the chains evenly (merged into one run per wave when the chains are back to back).
struct Group
{
  uint32_t begin, count;
  uint32_t flags; // 1: chains are single back-to-back rANS pieces (mergeable); 2: fill chains only (no table)
  uint32_t piece0; // mergeable groups: index of chain `begin`'s piece (chain begin + i is piece piece0 + i, its states are states[begin + i])
  uint64_t hist_off;
  uint64_t words_end; // first stream byte after the group's words (next group's first header) or the stream length
};
constexpr uint32_t kGroupMergeable = 1;
constexpr uint32_t kGroupFill = 2;

// A rank's sub-runs as ONE launch (hsrans_decode_sharded, round 6).  The reference hands every block of a stream to its pool in one
// pass and joins once (mt_rANS32x64_16w_decode.cpp:182-224, :262); a rank of a sharded decode used to queue one launch per sub-run
// so that sub-run k's ranges could go onto the links while sub-run k + 1 decodes — at 8 ranks x 4 sub-runs each launch was 32 MiB
// on a device that needs 100 MB to fill, and every one paid prologue, tail and kernel boundary.  Now the sub-runs ("parts":
// contiguous chain ranges of the rank's plan) are decoded by one launch in list order, and the launch itself tells the exchange's
// stream when a part is complete: a unit of work (a group of the grouped launch, a workgroup's share of the spread launch) that
// is done makes its stores visible (release fence, device scope), then counts itself into every part it overlaps
// (PartArgs::count, monotonic, never reset); the unit whose increment reaches `target` publishes `seq` to the part's completion
// word, which hipStreamWaitValue32(..., Gte) on the exchange's stream is waiting for.
constexpr uint32_t kMaxLaunchParts = 16;
struct PartArgs
{
  uint32_t n;                           // 0: not such a launch
  uint32_t seq;                         // what a completion word receives (one more with every launch of the sharded decode)
  uint32_t *count;                      // [n] units seen so far, over all launches
  uint32_t *done[kMaxLaunchParts];      // completion words (signal memory: the command processor polls them)
  uint32_t target[kMaxLaunchParts];     // count[k] once this launch's last unit of part k is in
  uint32_t chain_end[kMaxLaunchParts];  // part k = chains [chain_end[k - 1], chain_end[k]) of the launch's plan (the spread launch's units are chain ranges)
};
// grouped launches: Group::flags carries the first / last part a group overlaps in bits 16..23 / 24..31 (a group is a block or a
// part of one; sub-runs are cut at chain boundaries, so a group can straddle two of them)
constexpr uint32_t kGroupPartShift = 16;

// k_decode_dealt (kernels_dealt.h): its parameters beside the dealing (DealtTable, hsrans_launch.h)
struct DealtParams
{
  const uint8_t *stream;
  uint64_t stream_len, stream_lo;
  uint8_t *out;
  uint64_t out_cap;
  const Piece *pieces;    // chain c = piece c with start states c (single-piece chains)
  const uint32_t *states;
  uint32_t *status;
  uint64_t *stamps;       // diagnostics
  uint32_t n_chains, bits;
  uint16_t cum[2][17];    // a wave's part of its workgroup's share: cumulative class weights by grid half (as KParams::group_cum)
  uint32_t gap_chains;    // what the second prologue of a wave that straddles its share's block boundary costs, in chains of this plan (run_dealt)
  PartArgs parts;
};

// k_decode_single: a plan of ONE chain of ONE rANS piece (a raw stream without an index), filled by the host from the plan
struct SingleArgs
{
  uint32_t valid;        // 0: not such a plan (or bits == 15: its 8-byte table does not fit LDS)
  uint32_t steps, tail, S, bits, ring_entries;
  uint64_t hist_off, words_off, out_off;
};

struct KParams
{
  const uint8_t *stream; // device, 16-byte aligned: where stream byte 0 is (or would be: see stream_lo)
  uint64_t stream_len;
  uint64_t stream_lo;    // first stream byte that really exists at stream + offset (window launches; else 0)
  uint8_t *out; // device, 4-byte aligned
  uint64_t out_cap;
  const uint8_t *plan; // device copy of the plan blob
  uint32_t *status;    // device status word (kStatus* bits)
  // index-build pass only (ckpt_interval != 0): checkpoint g / ckpt_interval receives the S states and the absolute
  // byte position of the read cursor at group boundary g
  uint32_t *ckpt_states;
  uint64_t *ckpt_words;
  uint32_t ckpt_interval;
  // the same pass with explicit checkpoint positions: ascending absolute group indices; boundary k -> slot k
  const uint64_t *ckpt_groups;
  uint32_t n_ckpt_groups;
  // index-build pass over a block_ stream (walk plan): block b's header position, output offset and header word go to
  // walk_blocks[3b .. 3b+2], the coder states on entry to walk_states[b * S ..]; walk_count[0] = blocks seen
  uint64_t *walk_blocks;
  uint32_t *walk_states;
  uint32_t *walk_count;
  uint32_t walk_max_blocks;
  // diagnostics only (HSRANS_DEBUG_STAMPS=1): per wave {entry, table built, stream ready, done} s_memtime stamps; null otherwise
  uint64_t *stamps;
  PersistentArgs pa;
  const Group *groups; // null = not a grouped launch
  uint32_t n_groups;
  // grouped launches with more groups than workgroups: the groups behind the first gridDim.x are handed out by a ticket counter
  // (monotonic, this launch's own: never reset — every launch draws exactly n_groups tickets — see run_grouped); null = static
  unsigned long long *group_tickets;
  // calibration launches only (hsrans_ctx_calibrate): wave w of a one-chain-per-wave launch leaves its finish time (s_memrealtime,
  // 100 MHz) in finish[w]; finish[gridDim.x * waves] = the first wave's entry time
  uint64_t *finish;
  uint32_t spread;        // grouped plans of single-piece chains: the fewest chains of a coded block that is not the last (k_decode_spread takes the launch when its longest share is shorter); 0 = never
  uint32_t groups_lean;   // 64-state plan, every group a mergeable run or fills only: the lean instantiation of k_decode_grouped
  uint32_t group_prio;    // grouped launches: per mille of its run the younger half of a workgroup's waves decodes at raised priority (s_setprio)
  // ... per wave class (wave_class, kernels_layout.h): [0..7] where a group's chains are
  // split evenly over the waves, [8..9] (by grid half) where the split already follows the class weights.  All zero: group_prio's rule.
  uint16_t group_prio_class[10];
  // grouped launches: wave k of a workgroup in grid half h takes chains [count * cum[h][k] / cum[h][waves], count * cum[h][k+1] / cum[h][waves])
  // of its group (the same age-class weights as PersistentArgs::run_len)
  uint16_t group_cum[2][17];
  SingleArgs single;
  const uint32_t *single_states; // the chain's S start states (device)
  // private-table launches of 32-state plans: every wave takes TWO chains (2w, 2w+1), one per wave half, each with its own
  // table (run_private_pair); the LDS layout then holds two tables per wave
  uint32_t private_pair;
  PartArgs parts; // a sharded decode's sub-runs in one launch (k_decode_grouped<.., true, true>, k_decode_spread<.., true>); n == 0 otherwise
};

// ---- K independent streams in one launch (kernels_batch.h, hsrans_batch.cpp) -----------------------------------------------
// what is fixed when the batch is made: a member's plan, table and status word (device memory, read through the scalar cache)
struct BatchMember
{
  const Piece *pieces;
  const uint32_t *states;
  const uint2 *table;        // host-built decode table (MODE 3)
  const uint16_t *hist_copy; // the 256 counts it was built from
  uint32_t *status;          // the member's own status word (its device plan's)
  uint64_t hist_off;
  uint32_t n_chains, bits, S, reserved;
};
static_assert(sizeof(BatchMember) == 64, "BatchMember layout");
// one per wave of the launch: chains [begin, end) of member `member` are the wave's run (begin == end == n_chains: none)
struct BatchSlot
{
  uint32_t member, begin, end, flags;
};
constexpr uint32_t kBatchSlotCheckHist = 1; // the member's first workgroup: compares the table's histogram with the stream's
// what changes from launch to launch: where the member's stream and output are.  Passed as kernel arguments (no copy in front of
// the launch, graph-capturable), which bounds a launch at kBatchMax members; larger batches take several launches.
struct BatchIO
{
  const uint8_t *stream;
  uint64_t stream_len;
  uint8_t *out;
  uint64_t out_cap;
};
constexpr uint32_t kBatchMax = 32;
struct BatchParams
{
  BatchIO io[kBatchMax];
  const BatchMember *members;
  const BatchSlot *slots;
  uint64_t *finish; // diagnostics (batch stamps): wave w's finish time, [n_slots] = the first wave's entry; null otherwise
  uint64_t *stamps;
};
// the grouped form (block_/mt_ members with checkpoints): Group::flags carries the member from bit kGroupMemberShift up
constexpr uint32_t kGroupMemberShift = 16;
struct GroupMember
{
  const uint32_t *chain_first;
  const Piece *pieces;
  const uint32_t *states;
  uint32_t *status;
};
struct BatchGroupParams
{
  BatchIO io[kBatchMax];
  const GroupMember *members;
  const Group *groups; // all members' groups, flags |= member << kGroupMemberShift
  unsigned long long *tickets;
  uint32_t n_groups, bits, group_prio, reserved;
  uint16_t group_cum[2][17];
};
// (the two launches' shapes: batch_grouped_shape, batch_direct_shape)
hipError_t launch_batch_grouped(const BatchGroupParams &bp, const BatchGroupShape &shape, hipStream_t stream);
hipError_t launch_batch_direct(const BatchParams &bp, const BatchShape &shape, hipStream_t stream);

// K2: device-side walk of an mt_ stream's header chain (mt_rANS32x64_16w_decode.cpp:41-96), the device twin of the host
// planner.  Pass 1 (k_mt_chase, one wavefront) follows the chain with one 16-byte read per block and lists the blocks;
// pass 2 (k_mt_fill, one wavefront per block) writes the plan blob.
struct WalkResult
{
  uint32_t n_chains; // chains (= pieces = blocks) found
  uint32_t error;    // 0 ok; 7: the block list was too small; else the stream is malformed (the reference's "return 0" cases)
  uint64_t decoded_len;
};
hipError_t launch_mt_chase(const uint8_t *d_stream, uint64_t stream_len, uint64_t out_cap, uint32_t S, uint64_t *d_blocks, uint32_t max_blocks, WalkResult *d_result,
                           hipStream_t stream);
hipError_t launch_mt_fill(const uint8_t *d_stream, uint64_t stream_len, uint32_t S, uint32_t bits, const uint64_t *d_blocks, uint8_t *d_plan, uint32_t n_chains,
                          uint64_t out_len, WalkResult *d_result, hipStream_t stream);

// the indexed plan assembled on the device from a base plan + recorded checkpoints (hsrans_decode_device_indexing; kernels_walk.h)
// Few, large blocks (fewer groups than workgroup slots): a block's chains are cut into parts — groups of their own: same histogram,
// a sub-range of the chains — of at least kGroupPartChains chains until there are kGroupPartsPerCU parts per CU.  Round 4, in-process
// A/B on 100 MB (rotated, us; before: parts of >= 128 chains until two per CU): 256 KiB blocks 57.2 -> 51.3, 512 KiB 57.3 -> 53.2,
// 1 MiB 56.3 -> 52.1, 4 MiB 62.1 -> 51.1, 256 KiB at 13 bits 69.2 -> 58.1, at 15 bits 71.6 -> 62.2; parts of 48 or 32 chains lose again
// (profiles/r04_group_split_ab.txt).  Host (dplan_fill) and device (k_plan_blocks, k_index_fill) use the same rule.
constexpr uint32_t kGroupPartChains = 64, kGroupPartsPerCU = 3;
__host__ __device__ inline uint32_t group_parts_of(uint32_t chains, uint32_t k_max)
{
  const uint32_t by_size = chains / kGroupPartChains;
  const uint32_t k = by_size < k_max ? by_size : k_max;
  return k < 1 ? 1 : k;
}
// ... and the most parts a group is cut into in a plan of n_groups groups on a device that wants `want` of them (kGroupPartsPerCU per CU); 1 = no cut
__host__ __device__ inline uint32_t group_parts_max_of(uint64_t want, uint64_t n_groups)
{
  return n_groups != 0 && n_groups < want ? (uint32_t)((want + n_groups - 1) / n_groups) : 1;
}

// ---- the chains of an indexed plan: a block of T groups gets one chain per checkpoint -----------------------------------------------
// One rule for the host (hsrans_index_build, hsrans_decode_device_indexing's host assembly, cpu::index_build) and for the device
// (k_index_fill, k_walk_index_fill).  A block as the rule sees it:
struct IndexBlock
{
  uint64_t hist_off;  // its histogram in the stream; a single-symbol block: the symbol
  uint64_t words_off; // the read cursor at its first group
  uint64_t out_off;   // its first output byte
  uint64_t g0;        // ... as a group of the file (out_off / S)
  uint64_t fill_len;  // a single-symbol block: its bytes
  uint64_t T;         // whole groups it decodes
  uint32_t tail;      // symbols of the masked group behind them
  bool fill, last;    // a single-symbol block; the plan's last block
};
// ... from a base plan's piece (raw, mt_: one single-piece chain per block)
__host__ __device__ inline IndexBlock index_block_of_piece(const Piece &bp, uint32_t S, bool last)
{
  IndexBlock b{};
  b.hist_off = bp.hist_off;
  b.words_off = bp.words_off;
  b.out_off = bp.out_off;
  b.g0 = bp.out_off / S;
  b.fill_len = bp.fill_len;
  b.T = bp.steps;
  b.tail = bp.tail;
  b.fill = (bp.flags & kPieceFill) != 0;
  b.last = last;
  return b;
}
// ... from a record of the walk over a block_ stream {header position, output offset, header word}: a coded block stops at the file's last
// whole group (block_rANS32x64_16w_decode.cpp:82-88), and the file's tail belongs to the last block
__host__ __device__ inline IndexBlock index_block_of_walk(uint64_t pos, uint64_t at, uint64_t hdr, uint64_t decoded_len, uint32_t S, bool last)
{
  IndexBlock b{};
  b.out_off = at;
  b.g0 = at / S;
  b.fill = (hdr >> 63) != 0;
  b.last = last;
  if (b.fill)
  {
    b.hist_off = (hdr >> 54) & 0xFF;
    b.fill_len = hdr & (((uint64_t)1 << 54) - 1);
    return b;
  }
  b.hist_off = pos + 8;
  b.words_off = pos + 8 + 512;
  const uint64_t whole_file = decoded_len / S, e = (at + hdr + S - 1) / S, g1 = e < whole_file ? e : whole_file;
  b.T = g1 > b.g0 ? g1 - b.g0 : 0;
  b.tail = last ? (uint32_t)(decoded_len - whole_file * S) : 0;
  return b;
}
// a tail behind a trailing single-symbol block has no histogram: no plan
__host__ __device__ inline bool index_block_ends_short(const IndexBlock &b, uint64_t decoded_len) { return b.last && b.fill && b.out_off + b.fill_len < decoded_len; }
// its chains with a checkpoint every `interval` groups: group 0, interval, ... < T; at least group 0
__host__ __device__ inline uint32_t index_block_chains(const IndexBlock &b, uint32_t interval)
{
  return b.fill || b.T == 0 ? 1 : (uint32_t)((b.T + interval - 1) / interval);
}
// the checkpoint slot of its chain k: absolute group / interval, the group being g0 + k * interval
__host__ __device__ inline uint64_t index_chain_slot(const IndexBlock &b, uint32_t interval, uint64_t k) { return b.g0 / interval + k; }
// groups [g, g + steps) of the block as the one piece of chain `chain` of a plan, reading from words_off; the tail rides on the piece that
// ends the block
__host__ __device__ inline Piece index_sub_piece(const IndexBlock &b, uint32_t S, uint64_t g, uint64_t steps, uint64_t words_off, uint32_t chain)
{
  Piece p{};
  p.hist_off = b.hist_off;
  p.out_off = b.out_off + g * S;
  p.words_off = words_off;
  p.fill_len = b.fill_len;
  p.steps = (uint32_t)steps;
  p.tail = (uint16_t)(g + steps >= b.T ? b.tail : 0);
  p.flags = (uint16_t)(kPieceChainStart | (b.fill ? kPieceFill : 0));
  p.state_idx = chain;
  return p;
}
// the piece of its chain k, chain `chain` of the plan (ck_words[slot]: the read cursor a recording pass left at the checkpoint)
__host__ __device__ inline Piece index_chain_piece(const IndexBlock &b, uint32_t S, uint32_t interval, uint32_t k, const uint64_t *ck_words, uint32_t chain)
{
  const uint64_t g = b.fill ? 0 : (uint64_t)k * interval, left = b.T - g; // (a single-symbol block: its one chain is the whole block)
  uint64_t words_off = b.words_off;
  if (g != 0)
    words_off = ck_words[index_chain_slot(b, interval, k)];
  return index_sub_piece(b, S, g, b.fill || left < interval ? left : interval, words_off, chain);
}
// the S states chain k starts from: those the block is entered with, or the checkpoint's (ck_states[slot * S]); null: none (a fill, zeros)
__host__ __device__ inline const uint32_t *index_chain_states(const IndexBlock &b, uint32_t S, uint32_t interval, uint32_t k, const uint32_t *entry, const uint32_t *ck_states)
{
  return b.fill ? nullptr : k == 0 ? entry : ck_states + index_chain_slot(b, interval, k) * S;
}
// part `part` of `parts` of its `count` chains as a group of its own: chains [lo, hi), words up to the next part's first cursor (the last
// part: block_words_end)
struct IndexPart
{
  uint32_t lo, hi;
  uint64_t words_end;
};
__host__ __device__ inline IndexPart index_block_part(const IndexBlock &b, uint32_t interval, uint32_t count, uint32_t part, uint32_t parts, const uint64_t *ck_words,
                                                      uint64_t block_words_end)
{
  IndexPart r;
  r.lo = (uint32_t)((uint64_t)count * part / parts);
  r.hi = (uint32_t)((uint64_t)count * (part + 1) / parts);
  r.words_end = r.hi < count ? ck_words[index_chain_slot(b, interval, r.hi)] : block_words_end;
  return r;
}

// what the count kernels leave for the fill kernels and the host (in the new plan's arena: zeroed)
constexpr uint32_t kIndexNoFewest = 0xFFFFFFFFu;
struct IndexResult
{
  uint32_t chains;   // chains of the new plan
  uint32_t blocks;   // blocks they come from
  uint32_t coded;    // ... of them with a histogram: exactly one, and the plan's chains share its table (PlanBuilder::serialize)
  uint32_t fewest;   // fewest chains of a coded inner block (k_decode_spread's condition), kIndexNoFewest: there is none.  mt_: inner = not the
                     // last block; block_: neither the first nor the last coded block (as dplan_fill has it)
  uint64_t hist_off; // the last coded block's histogram
  uint32_t groups;   // groups of the grouped launch; 0: one chain per wave, no group list
  uint32_t parts;    // block_: parts a group is cut into at most
  uint32_t error;    // 0, or why there is no plan (1: the walk's block list, 2: a tail behind a single-symbol block, 3: more chains / groups than there is room for)
};
struct IndexArgs
{
  const uint8_t *base;       // base plan blob (device): one single-piece chain per mt_ block
  uint32_t n_base;           // its chains
  uint32_t S, interval;
  const uint32_t *ck_states; // [slot * S]: coder states at absolute group slot * interval
  const uint64_t *ck_words;  // [slot]: absolute stream byte of the read cursor there
  uint32_t *chain_off;       // [n_base] first chain of block b in the new plan (k_index_count)
  uint32_t *group_off;       // [n_base] first group of block b
  IndexResult *result;
  uint8_t *plan;             // the new plan blob (zeroed, sized for max_chains)
  uint32_t max_chains, max_groups; // what the plan blob and `groups` have room for
  Group *groups;             // [max_groups], zeroed
  uint32_t parts_want;       // kGroupPartsPerCU x CUs (group_parts_max_of)
  uint64_t stream_len;
};
hipError_t launch_index_assemble(const IndexArgs &a, hipStream_t stream);
// The same for a block_ stream, from what the recording walk left (KParams::walk_*): the plan hsrans_index_build(HSRANS_BLOCK) makes
// and the group list dplan_fill derives from it.  The block count is only known on the device: every buffer is sized by the host's bounds.
struct WalkIndexArgs
{
  const uint8_t *base;         // the walk plan's blob (device): container, states, bits and lengths come from its header
  const uint32_t *walk_count;  // blocks recorded; max_blocks + 1: the list overflowed
  const uint64_t *walk_blocks; // [3b .. 3b+2] = {header position, output offset, header word}
  const uint32_t *walk_states; // [b * S]: coder states on entry to block b
  const uint32_t *ck_states;   // as IndexArgs
  const uint64_t *ck_words;
  uint32_t S, interval;
  uint32_t max_blocks, max_chains, max_groups; // what walk_blocks, the plan blob and `groups` have room for
  uint32_t parts_want;         // kGroupPartsPerCU x CUs (group_parts_max_of)
  uint64_t decoded_len, stream_len;
  uint32_t *chain_off;         // [max_blocks] first chain of block b in the new plan (k_walk_index_count)
  uint32_t *group_off;         // [max_blocks] first group of block b
  IndexResult *result;
  uint8_t *plan;               // the new plan blob (zeroed, sized for max_chains)
  Group *groups;               // [max_groups], zeroed
};
hipError_t launch_index_assemble_walk(const WalkIndexArgs &a, hipStream_t stream);

// ---- the first decode of many streams in one call (kernels_index_batch.h, hsrans_capi_index_batch.cpp) ------------------------------
// what the recording pass needs of one member: a block_ stream's walk plan or an mt_ base plan, bound to its stream, output and buffers
struct IndexPassMember
{
  const uint8_t *stream; // device, 16-byte aligned
  uint64_t stream_len;
  uint8_t *out; // device, 4-byte aligned
  uint64_t out_cap;
  const uint8_t *plan;   // the base plan's blob (device)
  uint32_t *status;      // ... and its status word
  uint32_t *ck_states;   // KParams::ckpt_states / ckpt_words of this member
  uint64_t *ck_words;
  uint64_t *walk_blocks; // KParams::walk_* (null: an mt_ member)
  uint32_t *walk_states, *walk_count;
  uint32_t interval, walk_max_blocks;
};
static_assert(sizeof(IndexPassMember) == 96, "IndexPassMember layout");
// one wavefront's work: a walk member's one chain, or chain (block) `chain` of an mt_ member
struct IndexPassTask
{
  uint32_t member, chain;
};
constexpr uint32_t kIndexPassModes = 3; // the table layouts waves build for themselves: <= 11 bits, 12 bits, 13-15 bits
// tasks [0, n_tasks) at d_tasks, all of layout `mode`, the widest histogram among their members max_bits wide: one launch, one wavefront a task
hipError_t launch_index_pass_batch(int mode, uint32_t max_bits, const IndexPassTask *d_tasks, uint32_t n_tasks, const IndexPassMember *d_members, hipStream_t stream);
// count and fill for n members' argument structs at d_args; most_blocks: the largest n_base (max_blocks) among them; d_status_of[k]: member
// k's status word, copied to d_status_out[k] behind the pass
hipError_t launch_index_assemble_batch(const IndexArgs *d_args, uint32_t n, uint32_t most_blocks, const uint32_t *const *d_status_of, uint32_t *d_status_out, hipStream_t stream);
hipError_t launch_index_assemble_walk_batch(const WalkIndexArgs *d_args, uint32_t n, uint32_t most_blocks, const uint32_t *const *d_status_of, uint32_t *d_status_out,
                                            hipStream_t stream);
// 64-bit fingerprint of d_stream[0, stream_len) into *d_sum (16-byte aligned stream; asynchronous: memset + one launch)
hipError_t launch_stream_checksum(const uint8_t *d_stream, uint64_t stream_len, uint64_t *d_sum, hipStream_t stream);

// ---- byte ranges of one stream in one launch (kernels_gather.h, hsrans_capi_gather.cpp) --------------------------------------
// one wave's work: decoded bytes [begin, end) of the stream go to GatherParams::dst + byte + dst_delta
struct GatherTask // == hsrans_gather_task (include/hsrans_hip.h)
{
  uint64_t begin, end;
  int64_t dst_delta;
};
static_assert(sizeof(GatherTask) == 24, "GatherTask layout");
// what a gather wave needs of one planned stream, filled on the host from a device plan and the stream it is bound to (gather_source_of):
// the head of a gather set's member record (k_gather_set); k_gather and k_gather_ranges put it together from their parameters
struct GatherSource
{
  const uint8_t *plan; // the plan blob (device)
  uint32_t *status;    // ... and its status word
  const uint8_t *stream; // device, 16-byte aligned
  uint64_t stream_len;
  // plans with a host-built table (shared-table launches) only: the table, the counts it was made from and where the stream keeps them
  const uint2 *table;
  const uint16_t *hist_copy;
  uint64_t hist_off;
};
static_assert(sizeof(GatherSource) == 56, "GatherSource layout");
// (flat, in this order: with the GatherSource embedded k_gather<3, true> took 18.4 instead of 17.5 us per launch in tools/gather_batch_rate.py's
// single-call leg — the order decides which parameters the kernel loads together, and when)
struct GatherParams
{
  const uint8_t *stream; // device, 16-byte aligned
  uint64_t stream_len;
  uint8_t *dst; // device, any alignment
  const uint8_t *plan;
  uint32_t *status;
  const GatherTask *tasks; // device
  uint32_t n_tasks;
  // shared-table launches only: the plan's host-built table, the counts it was made from and where the stream keeps them
  const uint2 *table;
  const uint16_t *hist_copy;
  uint64_t hist_off;
};
// The rules of a range, once for the host entries and for k_gather_cut; none forms a sum that can wrap.
// [offset, offset + length) lies inside [0, extent): a range against its stream's decoded length, its destination against dst_capacity
__host__ __device__ inline bool gather_extent_ok(uint64_t offset, uint64_t length, uint64_t extent) { return offset <= extent && length <= extent - offset; }
// ... and a range that has bytes asks only for bytes the plan's chains write, [out_lo, out_hi) (a slice of a plan decodes part of the output)
__host__ __device__ inline bool gather_range_ok(uint64_t offset, uint64_t length, uint64_t dst_offset, uint64_t decoded_len, uint64_t out_lo, uint64_t out_hi, uint64_t dst_capacity)
{
  return gather_extent_ok(offset, length, decoded_len) && gather_extent_ok(dst_offset, length, dst_capacity) && (length == 0 || (offset >= out_lo && offset + length <= out_hi));
}
// the one-wave tasks of a range that is cut at the absolute multiples of the segment length (> 0)
__host__ __device__ inline uint64_t gather_range_tasks(uint64_t offset, uint64_t length, uint64_t segment)
{
  return length == 0 ? 0 : (offset + length - 1) / segment - offset / segment + 1;
}
// asynchronous on `stream`; one launch
hipError_t launch_gather(const GatherParams &gp, const GatherShape &shape, hipStream_t stream);

// ---- the same for ranges in device memory (hsrans_decode_device_gather_indirect): k_gather_cut, then k_gather_ranges ------------
struct GatherRange // == hsrans_range (include/hsrans_hip.h)
{
  uint64_t offset, length, dst_offset;
};
static_assert(sizeof(GatherRange) == 24, "GatherRange layout");
// the workspace, in uint32 words: what k_gather_cut leaves for k_gather_ranges
constexpr uint32_t kGatherWsTotal = 0;  // tasks of the launch; 0 where a range or the count was refused
constexpr uint32_t kGatherWsCount = 1;  // ranges in use: *count, or max_count
constexpr uint32_t kGatherWsFirst = 64; // first_task[0 .. count]: the tasks in front of range r (byte 256 of the workspace on)
struct GatherCutParams
{
  const GatherRange *ranges; // device, [max_count]
  const uint32_t *count;     // device or null (= max_count)
  uint32_t max_count;
  uint64_t segment; // the task length L (hsrans_gather_segment's rule), > 0
  uint64_t decoded_len, out_lo, out_hi, dst_capacity; // what a range is checked against
  uint32_t *workspace;
  uint32_t *status;
};
struct GatherRangesParams
{
  const GatherRange *ranges;
  const uint32_t *workspace;
  uint64_t segment;
  uint32_t segment_shift; // log2(segment) where it is a power of two, else 0: offset / segment without a division
};
// asynchronous on `stream`; two launches, nothing else (capturable)
hipError_t launch_gather_ranges(const GatherParams &gp, const GatherCutParams &cp, const GatherShape &shape, hipStream_t stream);

// ---- byte ranges of many streams, one launch per table layout (hsrans_decode_device_gather_batch): k_gather_set ------------------
// what a wave needs of the member its task belongs to: uploaded once per gather set, one record per member
struct GatherSetMember
{
  GatherSource src;
  uint64_t segment, decoded_len, out_lo, out_hi; // the member's task length L and what its ranges are checked against (the host's cut, and k_set_cut / k_set_ranges)
  uint32_t states, bits;
};
static_assert(sizeof(GatherSetMember) == 96, "GatherSetMember layout");
struct GatherSetTask // == hsrans_gather_batch_task (include/hsrans_hip.h)
{
  uint64_t begin, end;
  int64_t dst_delta;
  uint32_t member, reserved;
};
static_assert(sizeof(GatherSetTask) == 32, "GatherSetTask layout");
struct GatherSetParams
{
  const GatherSetMember *members; // device
  const GatherSetTask *tasks;     // device: the launch's entries, wave w of workgroup b runs entry b * waves + w
  uint32_t n_tasks;
  uint8_t *dst; // device, any alignment
  uint32_t table_bytes; // the largest table among the kind's members: what the LDS layout leaves room for per workgroup (shared) or wave (a multiple of 16)
};
// asynchronous on `stream`; one launch
hipError_t launch_gather_set(const GatherSetParams &sp, const GatherShape &shape, hipStream_t stream);

// ---- the same for ranges in device memory (hsrans_decode_device_gather_batch_indirect): k_set_cut, then k_set_ranges per kind ----
struct GatherSetRange // == hsrans_member_range (include/hsrans_hip.h)
{
  uint64_t offset, length, dst_offset;
  uint32_t member, reserved;
};
static_assert(sizeof(GatherSetRange) == 32, "GatherSetRange layout");
constexpr uint32_t kGatherKinds = 6; // the table layouts (kMode*): 0..2 a table per wave, 3..5 one per workgroup
// The workspace, in uint32 words: what k_set_cut leaves for the k_set_ranges launches.  A member's position is its place in kind-major
// order (members sorted by kind, then member index), so every kind owns a run of positions, of perm slots, of tasks and of units.
//   header     kSetWsTasks + k: tasks of kind k;  kSetWsUnits + k: units of kind k (3..5);  kSetWsSlot + k, k = 0..6: the first perm slot
//              of kind k (6: all slots);  kSetWsCount: ranges in use.  Every total is 0 where the call was refused.
//   slot_first [members + 1]    the perm slots in front of position p (while the ranges are counted: the ranges of p that have tasks)
//   unit_first [members + 1]    the units in front of position p (while the ranges are counted: the tasks of p); a unit is `waves`
//                               consecutive tasks of one member of a shared kind
//   cursor     [members]        where the scatter stands in p's slots
//   perm       [max_count]      the ranges that have tasks, by position
//   first_task [max_count + 1]  the tasks in front of perm slot s, over all kinds
constexpr uint32_t kSetWsTasks = 0, kSetWsUnits = 8, kSetWsSlot = 16, kSetWsCount = 24, kSetWsHeader = 64;
struct GatherSetWs
{
  uint64_t slot_first, unit_first, cursor, perm, first_task, words; // word offsets into the workspace (each a multiple of 64: 256 bytes), and its size
};
__host__ __device__ inline GatherSetWs gather_set_ws(uint32_t members, uint32_t max_count)
{
  const uint64_t per_pos = ((uint64_t)members + 1 + 63) & ~(uint64_t)63, per_range = ((uint64_t)max_count + 1 + 63) & ~(uint64_t)63;
  GatherSetWs w{};
  w.slot_first = kSetWsHeader;
  w.unit_first = w.slot_first + per_pos;
  w.cursor = w.unit_first + per_pos;
  w.perm = w.cursor + per_pos;
  w.first_task = w.perm + per_range;
  w.words = w.first_task + per_range;
  return w;
}
struct GatherSetCutParams
{
  const GatherSetRange *ranges; // device, [max_count]
  const uint32_t *count;        // device or null (= max_count)
  uint32_t max_count, n_members;
  const GatherSetMember *members; // device: a range is checked against its member's record and cut at its segment
  const uint32_t *position;       // device, [n_members]: the member's position
  uint64_t dst_capacity;
  uint32_t *workspace;
  uint32_t *status;                      // the set's own word
  uint32_t kind_first[kGatherKinds + 1]; // the first position of kind k ([6] = n_members)
  uint32_t kind_waves[kGatherKinds];     // waves per workgroup of kind k's launch (3..5: the length of a unit)
};
struct GatherSetRangesParams
{
  const GatherSetRange *ranges;
  const uint32_t *workspace;
  const GatherSetMember *members;
  uint8_t *dst;
  uint32_t max_count, n_members;
  uint32_t kind, pos_lo, pos_hi; // the launch's kind and its positions [pos_lo, pos_hi)
  uint32_t table_bytes;          // as GatherSetParams::table_bytes
};
// asynchronous on `stream`; one k_set_cut and one k_set_ranges per kind whose shape has a grid, nothing else (capturable)
hipError_t launch_gather_set_ranges(const GatherSetCutParams &cp, uint8_t *dst, const GatherShape shapes[kGatherKinds], const uint32_t table_bytes[kGatherKinds], hipStream_t stream);

// per device (call with the device current): raise the dynamic-LDS limit of every kernel variant to the gfx950 maximum
// (160 KiB) and report the device's geometry
hipError_t prepare_kernels(DeviceGeom *geom);
const char *kernel_name(KernelId k); // as rocprofv3 --kernel-trace prints it, without return type and parameter list
// `parts` (may be null): the launch decodes a rank's sub-runs and publishes a completion word per sub-run (PartArgs).  In: n,
// chain_end[], group_units[k] = groups of the plan's group list that overlap part k, cum[k] = the units counted into part k by all
// launches of this plan so far (the counters on the device are never reset).
struct PartPlan
{
  uint32_t n;
  const uint32_t *chain_end;
  const uint32_t *group_units;
  uint32_t *cum;
};
// asynchronous on `stream` of the current device; no allocation, no synchronisation (graph-capturable).
// facts (launch_facts) -> choice (choose_launch) -> the launch-dependent kernel parameters -> one launch through the kernel table ->
// *info from the choice.  `dealt` + `dealt_weights` (both or neither): the plan's shares for k_decode_dealt and the class weights
// they were dealt with (deal_shares).  `parts`: the units of the chosen kernel that overlap each part become its targets, cum[k] + units;
// cum[] itself moves only once the launch has been queued (hipSuccess), so a refused launch leaves host and device totals in step.
hipError_t launch_decode(const Tuning &tn, const KParams &kp, const PlanHeader &h, const DeviceGeom &dg, hipStream_t stream, LaunchInfo *info, const PartPlan *parts = nullptr,
                         const DealtTable *dealt = nullptr, const uint32_t *dealt_weights = nullptr);

} // namespace hsrans

#endif // HSRANS_KERNELS_H
