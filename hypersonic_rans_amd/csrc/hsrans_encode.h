// Launch interface of the gfx950 encoder (hsrans_encode.hip) for the C ABI (hsrans_capi.cpp).
#ifndef HSRANS_ENCODE_H
#define HSRANS_ENCODE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsrans
{

// one block of a chain encode (launch_encode_chain), in stream order; its image ends at scratch + slot_end
struct ChainBlock
{
  uint64_t begin, end;   // symbols [begin, end) of the input
  uint64_t slot_end;     // byte offset in scratch where the block's image ends
  uint64_t slot_bytes;   // encode_slot_bytes(end - begin, S): the slot below slot_end
  uint32_t ck_base;      // first checkpoint slot of the block (index_interval checkpoints)
  uint32_t single;       // 0x100 | symbol: single-symbol block (the 8-byte marker only); 0: coded with its counts in given_counts[b]
};

struct EncParams
{
  const uint8_t *in; // device, 16-byte aligned
  uint64_t n;
  uint8_t *out; // device, 16-byte aligned
  uint64_t out_cap;
  uint8_t *scratch;      // n_blocks slots of slot_bytes; a block's image ends at the end of its slot
  uint64_t slot_bytes;   // encode_slot_bytes()
  uint64_t *image_bytes; // [n_blocks] bytes of block b's image (header + words, or the 8-byte single-symbol marker)
  uint64_t *image_off;   // [n_blocks] position of the image in the stream
  uint64_t *fits;        // device memory: K_scan's copy of result[1] for K_gather (result may be page-locked host memory); unused up to kSelfScanBlocks blocks and by raw encodes
  uint64_t *result;      // [0] stream length, [1] 1 when it fits out_cap (else nothing is written to out), [2] chains,
                         // [3] blocks that are not single-symbol blocks, [4] position of the counts of the last such block
  uint64_t block;        // symbols per block (multiple of 64)
  uint32_t n_blocks;
  uint32_t S, bits;
  // sidecar plan (index_interval != 0 or a device plan was asked for)
  uint32_t interval;     // checkpoint every `interval` groups inside a block (multiple of 4; 0 = none)
  uint32_t max_ck;       // checkpoint slots per block
  uint32_t *ck_states;   // [n_blocks * max_ck * S] coder states at the checkpoints
  uint32_t *ck_pos;      // [n_blocks * max_ck] bytes between the decoder's read cursor at the checkpoint and the end of the block's words
  uint32_t *chain_count; // [n_blocks] chains of block b: 1 + its checkpoints (single-symbol block: 1)
  uint32_t *chain_off;   // [n_blocks] first chain of block b (K_scan)
  uint8_t *plan;         // plan blob to fill (K_plan) or null
  void *groups;          // Group[n_blocks * group_split] for the grouped decode launch (K_plan) or null
  uint32_t group_split;  // parts a block's chains are cut into (few large blocks: more workgroup tasks than blocks)
  uint32_t n_chains;     // total, known after K_scan (K_plan)
  // raw streams (launch_encode_raw): n_blocks = 1, block = n, one slot
  const uint32_t *raw_counts;   // raw: [256] byte counts of the input (k_raw_histogram's output), normalised by the coding wavefront;
                                // mt_: [n_blocks][256] byte counts per block, filled by k_block_histograms in launch_encode (null: every wavefront counts its own block)
  const uint16_t *given_counts; // [256] or null: the caller's normalised histogram (hist_t::symbolCount), used instead
  const uint32_t *ck_groups;    // or null: ascending group indices (multiples of 4) to checkpoint at, instead of `interval`
  uint32_t n_ck_groups;
  // chain encodes (launch_encode_chain): block_/mt_ streams whose states run through every block, one wavefront back to front
  const ChainBlock *chain_blocks; // [n_blocks]; given_counts then holds [n_blocks][256] normalised counts
  uint32_t chain_mt;              // 1: mt_ block headers {size, skip, states, counts}; 0: block_ {size, counts} and the states in the file header
  uint32_t chain_independent;     // 1: every block starts from fresh states (HSRANS_ENC_INDEPENDENT_BLOCKS)
  uint32_t *block_states;         // [n_blocks * S] or null: the decoder's states at each coded block's start (for the plan)
  uint64_t *stamps; // diagnostics (HSRANS_DEBUG_STAMPS=1): per block {start, histogram done, table done, words done} s_memrealtime; else null
};

uint32_t encode_block_count(uint64_t n, uint64_t block, uint32_t S); // 0: too many blocks
uint64_t encode_slot_bytes(uint64_t block, uint32_t S);
constexpr uint32_t kEncResultWords = 8;
// raises the dynamic-LDS limit of every encode kernel that needs more than the default, on the current device.  The attribute is per
// device, so each context calls it once, before its first encode of any kind; the launchers below rely on it
hipError_t prepare_encode_kernels();
// asynchronous on `stream`: K_enc, K_scan, K_gather.  cus: the device's CU count (picks the chunk variant)
hipError_t launch_encode(const EncParams &ep, uint32_t cus, hipStream_t stream);
// asynchronous on `stream`: [memset + K_hist ->] K_raw -> K_copy.  result[0] stream length, [1] fits out_cap, [2] listed checkpoints not met (0)
hipError_t launch_encode_raw(const EncParams &ep, uint32_t *d_counts, hipStream_t stream);
// asynchronous on `stream`: the unit summaries the block walk reads (hsrans_host.h UnitSummary, kUnitSummaryBytes each) of ep.n_blocks
// units of ep.block symbols (the last ends at ep.n) into `summaries`; with `log_table` (walk_log_table's, 2^bits + 1 floats, device
// memory) also every whole unit's fresh_cost, normalised at ep.block symbols
constexpr uint32_t kUnitSummaryBytes = 1040;
hipError_t launch_unit_summaries(const EncParams &ep, void *summaries, const float *log_table, hipStream_t stream);
// asynchronous on `stream`: K_chain (one wavefront, blocks back to front) -> K_gather_chain.  result[0] stream length, [1] fits
// out_cap, [2] listed checkpoints not met (0); image_off / image_bytes per block
hipError_t launch_encode_chain(const EncParams &ep, hipStream_t stream);
// asynchronous on `stream`: K_plan (needs ep.plan, ep.n_chains; after launch_encode's results are known)
hipError_t launch_encode_plan(const EncParams &ep, hipStream_t stream);

// ---- host pipeline (hsrans_encode_host_pipelined): one stream encoded slice by slice, a slice = a run of whole blocks ----
// Where the stream stands after the slices so far, in device memory; {16, 0, 0, 0} before the first
struct EncCarry
{
  uint64_t bytes_before;  // stream bytes so far (the 16-byte file header included)
  uint64_t chains_before; // plan chains so far
  uint64_t coded_blocks;  // blocks that are not single-symbol blocks
  uint64_t last_hist;     // position of the counts of the last such block
};
// asynchronous on `stream`: K_hist -> K_enc (launch_encode's) -> K_scan (carried) -> K_gather (carried).  ep describes the slice
// (ep.in its first byte, ep.n its length, ep.n_blocks its blocks; the per-block arrays start at its first block), ep.out its staging
// buffer (the images packed from byte 0); result[0..4] as launch_encode's, absolute, result[5] the stream position of the slice's first
// byte.  heads: or null, 16 + 4 S bytes per block of what k_plan_blocks reads of the images (launch_encode_plan_carried)
hipError_t launch_encode_slice(const EncParams &ep, EncCarry *carry, bool last_slice, uint8_t *heads, uint32_t cus, hipStream_t stream);
// asynchronous on `stream`: K_plan over the whole stream after its last slice, the images' heads at ep.scratch (launch_encode_slice's)
hipError_t launch_encode_plan_carried(const EncParams &ep, hipStream_t stream);

// mt_ streams of up to this many blocks: K_gather adds up the image sizes itself, beyond it K_scan runs first
constexpr uint32_t kEncSelfScanBlocks = 4096;

// ---- batches (hsrans_encode_device_batch): one workgroup of a batched launch works on block / part `index` (of `count`) of member `member`
struct EncTask
{
  uint32_t member, index, count;
};
// what launch_encode_batch launches, every array in device memory.  Raw members are as launch_encode_raw's EncParams (raw_counts: 256
// counts of their own inside `zero`), mt_ members as launch_encode's (raw_counts: their per-block counts; fits: a device word).
struct EncBatch
{
  const EncParams *params;     // [members]
  const EncTask *raw_parts;    // histogram and copy workgroups of the raw members: {member, part, parts}
  uint32_t n_raw_parts;
  const uint32_t *raw_members; // coding wavefronts: n_raw64 members of 64 states, then n_raw32 of 32
  uint32_t n_raw64, n_raw32;
  uint8_t *const *raw_headers; // [members]: where k_copy_images_batch puts a raw member's stream header for its plan, or null
  const EncTask *mt_blocks;    // every block of the mt_ members: {member, block, 0}, n_mt64_blocks of 64-state members first
  uint32_t n_mt64_blocks, n_mt32_blocks;
  const uint32_t *scan_members; // mt_ members of more blocks than k_gather_images adds up itself: K_scan's
  uint32_t n_scan;
  void *zero;                  // zeroed first (one memset): every member's result words and the raw members' counts
  size_t zero_bytes;
};
// asynchronous on `stream`: memset -> K_hist (raw), K_hist (mt_) -> K_raw per state count -> K_enc per state count -> [K_scan] -> K_gather
// -> K_copy; each kind launched once for all members, none for a kind no member needs.  *launches += the kernels launched
hipError_t launch_encode_batch(const EncBatch &batch, uint32_t cus, hipStream_t stream, uint32_t *launches);
// asynchronous on `stream`: K_plan over `tasks` (the mt_ blocks); members whose EncParams::plan is null are skipped
hipError_t launch_encode_plan_batch(const EncParams *params, const EncTask *tasks, uint32_t n_tasks, hipStream_t stream, uint32_t *launches);

// ---- batches of chain encodes (hsrans_encode_device_ex_batch) ----
// parts an image of a chain encode is copied in: about 1 MiB each of the stream's largest slot, so that few large adaptive blocks still spread over the device
inline uint32_t chain_gather_parts(uint64_t largest_slot_bytes)
{
  const uint64_t mib = largest_slot_bytes >> 20;
  return (uint32_t)(mib < 1 ? 1 : mib > 256 ? 256 : mib);
}
// one workgroup of the batched gather copies part `part` (of `parts`) of image `block` of member `member`
struct EncGatherTask
{
  uint32_t member, block, part, parts;
};
// asynchronous on `stream`: the unit summaries of many streams, every array in device memory.  params[m]: launch_unit_summaries' EncParams of
// member m; unit_tasks: {member, unit, 0} for every unit; cost_tasks: the same for the whole units of the members that walk the adaptive policy
// (none: no launch); summaries[m], log_tables[m]: where member m's summaries go, and walk_log_table's of its bit width (adaptive members)
hipError_t launch_unit_summaries_batch(const EncParams *params, const EncTask *unit_tasks, uint32_t n_unit_tasks, const EncTask *cost_tasks, uint32_t n_cost_tasks,
                                       uint8_t *const *summaries, const float *const *log_tables, hipStream_t stream, uint32_t *launches);
// asynchronous on `stream`: K_chain per state count present — members[0, n64) of 64 states, then n32 of 32, a workgroup of one wavefront
// each — then one K_gather_chain over `gather`.  params[m]: launch_encode_chain's EncParams of member m
hipError_t launch_encode_chain_batch(const EncParams *params, const uint32_t *members, uint32_t n64, uint32_t n32, const EncGatherTask *gather, uint32_t n_gather,
                                     hipStream_t stream, uint32_t *launches);

} // namespace hsrans

#endif // HSRANS_ENCODE_H
