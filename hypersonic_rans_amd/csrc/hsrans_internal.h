// hsrans_internal.h — what the translation units behind the C ABI (hsrans_capi*.cpp, hsrans_dplan.cpp, hsrans_batch.cpp, hsrans_comm.cpp) share: the
// context and device-plan objects behind the opaque handles of include/hsrans_hip.h, and the few helpers that work on them.
// Not installed; nothing outside csrc/ includes it.
#ifndef HSRANS_INTERNAL_H
#define HSRANS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/hsrans_hip.h"
#include "hsrans_carve.h"
#include "hsrans_encode.h"
#include "hsrans_host.h"
#include "hsrans_kernels.h"
#include "hsrans_planes.h" // PlanesRule

using namespace hsrans;

struct hsrans_dplan;
struct hsrans_hpipe;

struct hsrans_ctx
{
  int device = 0;
  char name[256] = {};
  DeviceGeom geom{};     // CU count / LDS of THIS context's device (nothing about a device is process-global)
  Tuning tuning = read_tuning(); // the switches as they were at hsrans_ctx_create: what the context's calls that make no object of their own use
  bool encoder_prepared = false; // prepare_encode_kernels has run for this context (encoder_ready: on its first encode, so a context that never encodes never loads the encoder)
  std::mutex lock; // guards the staging buffers of the host-pointer entries
  std::mutex stream_lock; // creation of pipe_streams (hsrans_hpipe_create may run under `lock` or without it)
  hipStream_t stream = nullptr;
  hsrans_dplan *host_dplan = nullptr; // device plan of the host-pointer entries, refilled per call (buffers are kept)
  // hsrans_decode_host without a plan (the plain decodeFunc): the index the first decode of a stream recorded, kept for the next
  // call on the same stream — {host address, length, codec, 64-bit fingerprint of all its bytes (computed on the device)}
  hsrans_dplan *host_index = nullptr;
  uint64_t host_index_key[4] = {};
  uint8_t host_index_head[128] = {}; // ... and the stream's first bytes, compared on the host first
  uint32_t host_index_head_len = 0;
  hsrans_hpipe *cached_pipe = nullptr; // hsrans_decode_host_pipelined: the pipeline of the plan used last
  uint64_t cached_pipe_key[3] = {};
  uint8_t *d_in = nullptr;
  size_t d_in_cap = 0;
  uint8_t *d_out = nullptr;
  size_t d_out_cap = 0;
  uint8_t *d_plan = nullptr;
  size_t d_plan_cap = 0;
  uint32_t *d_status = nullptr;
  uint8_t *d_enc_scratch = nullptr; // the GPU encoders' block images (slots)
  size_t d_enc_scratch_cap = 0;
  uint8_t *d_enc_meta = nullptr;
  size_t d_enc_meta_cap = 0;
  uint8_t *d_enc_ck = nullptr; // checkpoint states / cursors of the blocks being encoded
  size_t d_enc_ck_cap = 0;
  // the three streams of the host pipelines (upload / decode / download): created once and shared by every hsrans_hpipe of the
  // context.  Streams made per pipe were a trap: the second pipe of a process got streams on ONE hardware queue, its uploads and
  // kernels ran one after the other, and every codec after the first in the harness read 24-26 instead of 33 GiB/s.
  hipStream_t pipe_streams[3] = {nullptr, nullptr, nullptr};
  uint64_t *h_enc_result = nullptr; // page-locked, device-mapped: hsrans_encode_device's kernels write their result words straight into it (no copy kernel, no second launch gap); under `lock`
  uint8_t *h_pin = nullptr; // page-locked staging of hsrans_decode_device_indexing (checkpoints down, plan blob up); under `lock`
  size_t h_pin_cap = 0;
  // hsrans_decode_device_gather's task lists (hsrans_capi_gather.cpp), under `lock`: a page-locked host buffer and its device twin, used as
  // two halves by region; gather_ev[k] = the last launch that read half k
  uint8_t *d_gather = nullptr, *h_gather = nullptr;
  size_t d_gather_cap = 0, h_gather_cap = 0, gather_cursor = 0;
  hipEvent_t gather_ev[2] = {nullptr, nullptr};
  bool gather_ev_used[2] = {false, false}, gather_have_last = false;
  hipStream_t gather_last_stream = nullptr;
  uint32_t gather_last_half = 0;
  uint8_t *h_pipe_result = nullptr; // page-locked, device-mapped: hsrans_encode_host_pipelined's carry start and per-slice result words; under `lock`
  size_t h_pipe_result_cap = 0;
};

// every device plan (and every refill of one) has a number of its own: what hsrans_queue keys its cached batches by — an address can come back
// with another plan behind it
inline uint64_t next_dplan_uid()
{
  static std::atomic<uint64_t> n{1};
  return n.fetch_add(1, std::memory_order_relaxed);
}

// What a fill derives from the plan it launches.  Every (re)fill resets all of it in one assignment (dplan_fill), so no field here can carry
// one plan's launch state into the next.
struct DplanState
{
  uint64_t uid = next_dplan_uid(); // (a refill is another plan)
  Tuning tuning = read_tuning();   // the switches as they were at this fill or dplan_adopt: what the plan's launches use
  PlanHeader hdr{};
  size_t plan_bytes = 0;
  // regions of d_arena (dplan_arena): not freed one by one
  uint8_t *d_plan = nullptr;
  uint32_t *d_status = nullptr;
  unsigned long long *d_counters = nullptr; // uniform persistent launches: kCounterSets sets of monotonic queue heads
  uint8_t *d_table = nullptr;               // host-built decode table (plans that carry their histogram)
  uint8_t *d_groups = nullptr;              // grouped launches (block_/mt_ plans with checkpoints)
  uint32_t n_groups = 0;
  bool groups_lean = false; // 64 states, every group a mergeable run or fills only
  uint32_t spread_min_block = 0; // plans k_decode_spread can take (single-piece chains, mergeable / fill groups): the fewest chains of a coded block that is not the last; else 0
  PersistentArgs pa{};
  SingleArgs single{};
  // what the plan's chains touch, recorded by dplan_fill: the lowest stream byte any of them reads (its own words, its
  // histogram / header, the shared histogram when the plan carries no copy of it) and the output bytes they write
  uint64_t body_lo = 0, out_lo = 0, out_hi = 0;
  // part_units[k]: the groups that count into sub-run k of part_ends (below); part_cum[k] = units counted into part k by all launches so far
  // (the device's counters are never reset: launch_decode, PartPlan)
  std::vector<uint32_t> part_units, part_cum;
  // k_decode_dealt (kernels_dealt.h): the plan's blocks as chain ranges — block k = chains [block_begin[k], block_begin[k + 1]) — kept where the
  // plan is a lean grouped one of coded blocks only (no single-symbol blocks); empty otherwise.  `dealt` = the shares for `dealt_weights`
  // (dealt_state 1: valid, -1: the plan does not suit the launch with these weights, 0: not dealt yet); re-dealt when a calibration changes the weights.
  // hsrans_queue: raw plans whose chains start at the same groups are dealt alike in a batch launch — a hash over (states, bits, chain count,
  // every chain's groups), taken when the plan is filled from its host blob; 0 = none (plans written on the device, other containers)
  uint64_t deal_sig = 0;
  std::vector<uint32_t> block_begin;
  DealtTable dealt{};
  uint32_t dealt_weights[8] = {};
  int dealt_state = 0;
};

// A device plan.  Every one comes from dplan_new and holds its device memory in ONE allocation, d_arena (a device plan used to cost up to
// five hipMalloc calls and three synchronisations: 3.2 ms for a 2.5 MB index); hsrans_dplan_destroy frees d_stamps and d_arena.
struct hsrans_dplan : DplanState
{
  hsrans_ctx *ctx = nullptr;
  uint8_t *d_arena = nullptr;
  size_t d_arena_cap = 0;
  uint64_t *d_stamps = nullptr; // diagnostics (HSRANS_DEBUG_STAMPS=1)
  uint64_t *d_finish = nullptr; // hsrans_ctx_calibrate: per-wave finish times of the plan's launches (owned by the calibration)
  std::atomic<uint32_t> epoch{0}; // launches so far: launch k uses counter set k % kCounterSets
  // a rank's sub-runs decoded by ONE launch of this plan (hsrans_comm.cpp): part k = chains [part_ends[k - 1], part_ends[k]) — set before
  // dplan_fill, which then tags every group with the parts it overlaps (Group::flags, kGroupPartShift) and counts them: part_units
  std::vector<uint32_t> part_ends;
  LaunchInfo info{};
};

// a fresh device plan of ctx (with the stamps buffer when HSRANS_DEBUG_STAMPS is set: Tuning::debug_stamps); null when out of memory
hsrans_dplan *dplan_new(hsrans_ctx *ctx);
// hsrans_dplan_create; part_ends (may be null): the chains [part_ends[k - 1], part_ends[k]) are the sub-runs of a sharded decode
// (hsrans_comm.cpp), and the group list is tagged with them.  *out_dplan's part_units is empty when the plan is of a kind no one-launch kernel takes.
int dplan_create(hsrans_ctx *ctx, const uint8_t *plan, size_t plan_size, const std::vector<uint32_t> *part_ends, hsrans_dplan **out_dplan);

// The regions of a plan's device memory, in this order, each 256-byte aligned: status word, ticket counters, plan blob, host-built table,
// group list, caller scratch.  An empty region's pointer is null (the status word and the plan are always there).
enum DplanZero { kZeroThroughCounters, kZeroThroughPlan, kZeroAll };
struct DplanRegions
{
  bool counters = false;
  size_t plan = 0, table = 0, groups = 0, scratch = 0; // bytes
  DplanZero zero = kZeroThroughCounters; // what starts at zero (one memset on the caller's stream)
};
// lays them out in d_arena (kept and grown across refills), sets the d_* pointers and epoch, queues the memset; *scratch: the caller's region
int dplan_arena(hsrans_dplan *d, const DplanRegions &r, hipStream_t s, uint8_t **scratch = nullptr);
// takes over a plan the device wrote into d's arena: its header, its group count (0: ungrouped, groups and counters are dropped) and the fewest
// chains of a coded block that is not the last; fills block_begin from the group list (synchronises `s` when there is one)
// host_groups (may be null): the caller's copy of the first n_groups groups, already on the host — nothing is copied and nothing synchronised
void dplan_adopt(hsrans_dplan *d, const PlanHeader &h, uint32_t n_groups, uint64_t spread_min_block, hipStream_t s, const Group *host_groups = nullptr);
// the header of an mt_ plan written on the device (the GPU encoder's, K2's): n_chains single-piece chains
PlanHeader mt_plan_header(uint32_t states, uint32_t bits, uint64_t decoded_len, uint64_t stream_len, uint32_t n_chains);

// Few, large blocks would leave workgroup slots empty (one workgroup per group): while a plan has fewer groups than kGroupPartsPerCU per CU,
// each is cut into up to this many parts of >= kGroupPartChains chains (hsrans_kernels.h group_parts_of: the rule and what was measured); 1 = no cut
inline uint32_t group_parts_max(const DeviceGeom &geom, size_t n_groups)
{
  return group_parts_max_of((uint64_t)kGroupPartsPerCU * geom.num_cus, n_groups);
}

constexpr size_t kStampWaves = 16384;

inline bool grow(uint8_t **p, size_t *cap, size_t need)
{
  if (need <= *cap)
    return true;
  if (*p)
    (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = need + need / 8 + 4096;
  if (hipMalloc((void **)p, want) != hipSuccess)
  {
    (void)hipGetLastError(); // (consumed here: the runtime's last error is sticky per thread and would surface at an unrelated launch)
    return false;
  }
  *cap = want;
  return true;
}

inline bool grow_pinned(uint8_t **p, size_t *cap, size_t need)
{
  if (need <= *cap)
    return true;
  if (*p)
    (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = need + need / 4 + 65536;
  if (hipHostMalloc((void **)p, want, hipHostMallocDefault) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  *cap = want;
  return true;
}

// page-locked and mapped into the device's address space (hipHostGetDevicePointer)
inline bool grow_pinned_mapped(uint8_t **p, size_t *cap, size_t need)
{
  if (need <= *cap)
    return true;
  if (*p)
    (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = need + need / 4 + 4096;
  if (hipHostMalloc((void **)p, want, hipHostMallocMapped) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  *cap = want;
  return true;
}

inline bool read_header(const uint8_t *plan, size_t size, PlanHeader *h)
{
  if (plan == nullptr || size < sizeof(PlanHeader))
    return false;
  memcpy(h, plan, sizeof(PlanHeader));
  return memcmp(h->magic, "HSRPLAN1", 8) == 0;
}

struct hsrans_batch
{
  hsrans_ctx *ctx = nullptr;
  Tuning tuning = read_tuning(); // (at hsrans_dplan_batch_create: the shapes and weights of its launches)
  std::vector<hsrans_dplan *> members;
  struct DirectLaunch
  {
    std::vector<uint32_t> member_idx; // batch member of launch-local member i
    BatchShape shape{};
    const BatchMember *d_members = nullptr;
    const BatchSlot *d_slots = nullptr;
    double imbalance = 1.0;
  };
  std::vector<DirectLaunch> direct;
  // block_/mt_ members with checkpoints (64 states, one width <= 12 bits per launch): all their groups in ONE k_decode_grouped_batch launch
  struct GroupedLaunch
  {
    std::vector<uint32_t> member_idx;
    BatchGroupShape shape{};
    const GroupMember *d_members = nullptr;
    const Group *d_groups = nullptr;
    unsigned long long *d_tickets = nullptr; // kCounterSets monotonic ticket counters, one per launch in flight (as a device plan's)
    uint32_t n_groups = 0, bits = 0;
    std::atomic<uint32_t> *epoch = nullptr; // (heap: the struct must stay movable)
  };
  std::vector<GroupedLaunch> grouped;
  std::vector<uint32_t> solo; // members that take a launch of their own (hsrans_decode_device's)
  uint8_t *d_arena = nullptr;
  // per-wave finish times of the first shared launch: diagnostics (HSRANS_BATCH_STAMPS=1: owned by the batch) and
  // hsrans_ctx_calibrate_runs (which points it at its own buffer launch by launch: finish_owned false)
  uint64_t *d_finish = nullptr;
  bool finish_owned = false;
  uint32_t finish_slots = 0;
  std::vector<uint32_t> order_run; // per member: the slot order its chains were dealt with (diagnostics)
};

// hsrans_planes (hsrans_capi_planes.cpp): a frame's descriptor bound to its planes' device plans; hsrans_capi_planes_gather.cpp reads it
struct hsrans_planes
{
  hsrans_ctx *ctx = nullptr;
  hsrans_planes_desc desc{};
  hsrans_batch *batch = nullptr;   // over the coded planes; null when every plane is stored
  std::vector<uint32_t> coded;     // plane of batch member k
  std::vector<hsrans_dplan *> dplans; // of the coded planes, in batch order
};

// hsrans_planes_set (hsrans_capi_planes_batch.cpp): many frames' descriptors bound to their planes' device plans;
// hsrans_capi_planes_gather_batch.cpp reads it
struct hsrans_planes_set
{
  hsrans_ctx *ctx = nullptr;
  std::vector<hsrans_planes_desc> descs;
  hsrans_batch *batch = nullptr;      // over the coded planes of all members; null when every plane is stored
  std::vector<uint32_t> coded_member; // member and plane of batch member j
  std::vector<uint32_t> coded_plane;
  std::vector<hsrans_dplan *> coded_plans; // ... and its plan
  std::vector<size_t> work_at;        // [count + 1]: the members' regions of the workspace, then its size
  std::vector<uint32_t> first_task;   // [count + 1]: the merge's task prefix, then its total
  uint32_t batch_launches = 0;
};

// What hsrans_encode_device_planes and every member of hsrans_encode_device_planes_batch share (hsrans_capi_planes.cpp): the single call's
// rules for one tensor but the workspace's and the overlap rule — element size, flags, d_in and d_frame set and 16-byte aligned, states,
// elements, each plane by mt_shape, frame_capacity >= elem_size * stride.  *out: a coded plane's room in the frame, a plane's room in the
// workspace, a plane's mt_ blocks.
struct PlanesEncShape
{
  size_t stride = 0, work_stride = 0;
  uint32_t n_blocks = 0;
};
bool planes_encode_check(uint32_t W, int states, uint32_t bits, const void *d_in, size_t elements, const void *d_frame, size_t frame_capacity, uint32_t block_size,
                         uint32_t index_interval, uint32_t flags, bool want_plans, PlanesEncShape *out);
// hsrans_planes_create's rules for a descriptor and its planes' plans (dplans[p] null exactly for the stored planes): HSRANS_OK or HSRANS_E_ARG
int planes_desc_check(const hsrans_ctx *ctx, const hsrans_planes_desc *desc, hsrans_dplan *const *dplans);

// ---- what the plain byte-plane entries and their delta forms (hsrans_*_device_planes_delta, each beside its plain entry) share: each plain
// entry's whole body, taking an optional base.  Without one (`on` false) a flow is the plain entry, check for check and launch for launch;
// with one the launcher is handed the base, so the split or the merge is the delta kernel (hsrans_planes_base.hip), and the base joins the checks.  Hidden: the library's exported symbols are the header's.
// The diff forms (hsrans_*_device_planes_diff) are the delta forms with the other residue rule: the same flows, checks, spans, refusals and
// launch counts, the launcher handed PlanesRule::kDiff, so the kernel is that unit's _diff one. ----
struct PlanesBase
{
  bool on = false; // a delta or diff call (a plain one never looks at the rest)
  const void *d = nullptr;
  size_t bytes = 0;
  PlanesRule rule = PlanesRule::kXor; // what the planes hold of the tensor and the base (hsrans_planes.h)
};
// The base's own checks and its part in the overlap rule: set, 16-byte aligned, at least W * elements bytes (false otherwise); a read span,
// pushed onto *spans.  d_out (null: the call has no in-place form): where the output is exactly the base — the same address, out_capacity
// within the base's bytes — the output's span stands for those bytes and only the base's remainder behind it is pushed.
__attribute__((visibility("hidden"))) bool planes_base_spans(const PlanesBase &base, uint32_t W, size_t elements, const void *d_out, size_t out_capacity,
                                                             std::vector<Span> *spans);
// A decode reads its frame, and by the overlap rule two reads may share; a base may still not meet the frame it is decoded against (a base
// over compressed bytes is never a meaningful call): whether base.d over base.bytes intersects the frame.  False without a base.
__attribute__((visibility("hidden"))) bool planes_base_meets_frame(const PlanesBase &base, const void *d_frame, size_t frame_length);
// hsrans_encode_device_planes, hsrans_decode_device_planes (hsrans_capi_planes.cpp)
__attribute__((visibility("hidden"))) size_t planes_encode_flow(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const PlanesBase &base,
                                                                size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval,
                                                                uint32_t flags, void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc,
                                                                hsrans_dplan **out_dplans);
__attribute__((visibility("hidden"))) int planes_decode_flow(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const PlanesBase &base,
                                                             void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
// hsrans_encode_device_planes_batch, hsrans_decode_device_planes_batch (hsrans_capi_planes_batch.cpp); delta: d_bases and base_bytes are
// arrays of one entry per member, a null d_bases[k] a member without a base; rule: the one residue rule of all members with a base
__attribute__((visibility("hidden"))) int planes_encode_batch_flow(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases, const size_t *base_bytes,
                                                                   bool delta, PlanesRule rule, uint32_t count, void *d_work, size_t work_bytes, void *hip_stream,
                                                                   hsrans_dplan **out_dplans, hsrans_planes_batch_stats *stats);
__attribute__((visibility("hidden"))) int planes_decode_batch_flow(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                                                   const void *const *d_bases, const size_t *base_bytes, bool delta, PlanesRule rule, void *const *d_outs,
                                                                   const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream);
// hsrans_decode_device_planes_gather (hsrans_capi_planes_gather.cpp); no in-place form
struct hsrans_planes_gather;
__attribute__((visibility("hidden"))) int planes_gather_flow(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const PlanesBase &base,
                                                             void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
// hsrans_decode_device_planes_gather_indirect (hsrans_capi_planes_gather.cpp): with a base the merge is k_planes_merge_indirect_delta
// (hsrans_planes_gather_delta.hip), and the base keeps clear of the frame, the ranges and the count word as well as of what is written
__attribute__((visibility("hidden"))) int planes_gather_indirect_flow(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges, const uint32_t *d_count,
                                                                      uint32_t max_count, uint64_t max_elements, const PlanesBase &base, void *d_out, size_t out_capacity,
                                                                      void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes, void *hip_stream);
// hsrans_decode_device_planes_gather_batch and _gather_batch_indirect (hsrans_capi_planes_gather_batch.cpp); bs: null (the plain call), or a
// base set of this gather set and context, one base per member: the merges are then the table-driven ones of hsrans_planes_gather_delta.hip
struct hsrans_planes_gather_set;
struct hsrans_planes_base_set;
__attribute__((visibility("hidden"))) int planes_gather_batch_flow(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs,
                                                                   const hsrans_member_range *ranges, uint32_t count, void *d_out, size_t out_capacity, void *d_work,
                                                                   size_t work_bytes, void *hip_stream);
__attribute__((visibility("hidden"))) int planes_gather_batch_indirect_flow(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs,
                                                                            const hsrans_member_range *d_ranges, const uint32_t *d_count, uint32_t max_count, void *d_out,
                                                                            size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes,
                                                                            void *hip_stream);

// (Re)fills a device plan from a validated host plan blob; one launch of a filled device plan (hsrans_dplan.cpp)
int dplan_fill(hsrans_dplan *d, const uint8_t *plan, size_t plan_size, const PlanHeader &h, hipStream_t s);
int dplan_launch(hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity, hipStream_t s, uint64_t stream_lo = 0,
                 const PartArgs *part_words = nullptr);

// hsrans_decode_device_ranges' body: stream bytes [window_offset, +window_length) at d_window, output bytes [out_offset, +out_length) at d_out;
// part_words: a sharded decode's sub-runs in this one launch (completion words, sequence number; hsrans_comm.cpp)
int dplan_launch_ranges(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_window, size_t window_offset, size_t window_length, void *d_out, size_t out_offset,
                        size_t out_length, void *hip_stream, const PartArgs *part_words);

// ---- the GPU encoder's host side (hsrans_capi_encode.cpp): what hsrans_encode_device_raw, hsrans_encode_device, hsrans_encode_device_batch
// and hsrans_encode_host_pipelined share, so that a batch member gets exactly what its single call would ----

// under ctx->lock: the context's device made current and, on the context's first encode of any kind, prepare_encode_kernels run
bool encoder_ready(hsrans_ctx *ctx);
inline bool device_io_ok(const void *d_in, const void *d_out) // a device encode's input and output: set and 16-byte aligned
{
  return d_in != nullptr && d_out != nullptr && ((uintptr_t)d_in & 15) == 0 && ((uintptr_t)d_out & 15) == 0;
}
// the context's three encoder buffers, each grown to at least its size: block images (slots), per-call records, checkpoints
bool encoder_buffers(hsrans_ctx *ctx, size_t scratch, size_t meta, size_t ck);
// the checkpoint region of an encode with ck_slots slots of S states: [ck_slots][S] states, then ck_slots positions (32-bit words both)
inline size_t ck_region_bytes(size_t ck_slots, uint32_t S) { return ck_slots * ((size_t)S * 4 + 4); }
void ck_region(EncParams *ep, uint8_t *at, size_t ck_slots, uint32_t S); // ep->ck_states, ep->ck_pos
// Synchronises `s` whether or not everything before it was queued (what was queued may still read the caller's host buffers); on a failure of
// either kind the runtime's sticky error is consumed.  True: all was queued and has run.
bool stream_settle(hipStream_t s, bool queued);
// the status of a byte-plane gather object all of whose planes were stored: no plan has anything to report, but the call still waits for the
// stream as the gather set's status call does
inline int planes_all_stored_status(hsrans_ctx *ctx, void *hip_stream)
{
  return hipSetDevice(ctx->device) == hipSuccess && stream_settle((hipStream_t)hip_stream, true) ? HSRANS_OK : HSRANS_E_HIP;
}
// an encode's result words (EncParams::result): word 1, it was coded and fitted d_out; with check_refusal also word 2, the listed checkpoints
// the pass did not meet, which must be 0.  The one-wavefront-per-block mt_ encodes keep their chain count in word 2: no check_refusal there.
inline bool enc_result_ok(const uint64_t *result, bool check_refusal) { return result[1] == 1 && (!check_refusal || result[2] == 0); }
// what an encode of one raw or mt_ stream derives from its arguments before anything is launched
struct EncShape
{
  uint32_t S = 0, bits = 0;
  uint64_t n = 0, block = 0; // input bytes; symbols per block (raw: n)
  uint32_t n_blocks = 1;
  uint64_t slot_bytes = 0;   // per block (raw: the one slot)
  uint32_t interval = 0;     // EncParams::interval
  uint32_t max_ck = 0;       // EncParams::max_ck
  size_t ck_slots = 1;       // checkpoint slots of the whole stream
  // raw only
  bool listed = false;    // checkpoints at the caller's groups rather than every `interval`
  bool want_plan = false; // a plan was asked for and the stream gets checkpoints
  size_t n_ck = 0;        // checkpoints the pass records
  EncParams params(const void *d_in, void *d_out, size_t out_capacity) const; // the fields above, the input and the output
};
// the rules of a raw encode (hsrans_encode_device_raw's) but the pointers'; plan: a plan is asked for
bool raw_shape(int states, uint32_t bits, size_t length, size_t out_capacity, const hsrans_hist *hist, uint32_t index_interval, const uint64_t *index_groups,
               size_t n_index_groups, bool plan, EncShape *sh);
// the rules of an mt_ encode in blocks of block_size symbols (hsrans_encode_device's) but the pointers'; plan: a plan is asked for (checkpoints only serve it)
bool mt_shape(int states, uint32_t bits, size_t length, size_t out_capacity, uint32_t block_size, uint32_t index_interval, bool plan, EncShape *sh);
// an mt_ stream's per-block arrays, laid out at `at` (16-byte aligned) for ep->n_blocks blocks: image_bytes, image_off [nb] u64, chain_count,
// chain_off [nb] u32, fits (16 bytes, 16-byte aligned), raw_counts [nb][256] u32 (16-byte aligned)
size_t mt_block_arrays_bytes(uint32_t n_blocks);
void mt_block_arrays(EncParams *ep, uint8_t *at);
// the header of an mt_ stream's plan from its encode's result words (EncParams::result) and ep's S, bits, n and interval; false: no plan in them
bool mt_result_header(const EncParams &ep, const uint64_t *result, PlanHeader *h);
// the device plan K_plan writes for an mt_ encode: its header (mt_result_header), the group split (ep->group_split), the plan object with the
// header copied in on `s`, and ep->plan / groups / n_chains pointed at it; null on failure.  *h must live until `s` is synchronised.
hsrans_dplan *mt_plan_begin(hsrans_ctx *ctx, EncParams *ep, const uint64_t *result, PlanHeader *h, hipStream_t s);
// after K_plan (and `s` synchronised): the plan object takes over what the device wrote
void mt_plan_adopt(hsrans_dplan *d, const EncParams &ep, const PlanHeader &h, hipStream_t s);
// a raw encode's plan (what hsrans_encode_ex emits) from what came down: the stream's first 16 + 512 + 4 S bytes and the checkpoints' states and
// positions, at sh's listed groups (index_groups) or every sh.interval.  Into plan_out (null: a buffer of its own); then *plan_size and, with
// out_dplan, a device plan of it.  Returns the plan's size, 0 on failure.
size_t raw_plan(hsrans_ctx *ctx, const EncShape &sh, uint64_t total, const uint64_t *index_groups, const uint8_t *header, const uint32_t *ck_states,
                const uint32_t *ck_pos, uint8_t *plan_out, size_t plan_capacity, size_t *plan_size, hsrans_dplan **out_dplan);

// ---- the chain path (hsrans_capi_encode.cpp): what hsrans_encode_device_ex and hsrans_encode_device_ex_batch share, step by step ----
// where hsrans_encode_device_ex sends its arguments (the context and the histogram aside); kExRefused: it returns 0
enum ExRoute
{
  kExRefused,
  kExRaw,        // hsrans_encode_device_raw
  kExBlocks,     // hsrans_encode_device, no plan
  kExBlocksPlan, // hsrans_encode_device with checkpoints every interval, its plan read back
  kExChain       // the chain: unit summaries, the host walk, one coding wavefront, the gather
};
// One stream on its way through the chain path: the arguments (ex_route), the summaries request (chain_units), the blocks (chain_walk)
// and what the coding wavefront and the plan need of them (chain_prepare)
struct ChainJob
{
  int container = 0;
  uint32_t S = 0, bits = 0;
  const void *d_in = nullptr;
  size_t length = 0;
  void *d_out = nullptr;
  size_t out_capacity = 0;
  size_t block = 0; // fixed blocks of this many symbols; 0: the adaptive policy
  bool fixed = false, independent = false, want_plan = false;
  uint32_t interval = 0; // checkpoints every `interval` groups (0 with listed ones)
  const uint64_t *ig = nullptr; // listed checkpoints, or null
  size_t n_ig = 0;
  size_t unit = 0, n_units = 0; // chain_units: the summaries' unit (the fixed block, or walk_unit) and their number
  std::vector<BlockSpan> spans; // chain_walk
  // chain_prepare
  std::vector<ChainBlock> cb;
  std::vector<uint16_t> counts;  // [blocks][256]: the normalised counts of the coded blocks
  std::vector<uint32_t> ck_list; // listed checkpoints the host encoder meets (inside a coded block, not its first group, below the file's whole groups)
  std::vector<uint32_t> ck_block; // the block of every checkpoint slot
  uint32_t n_ck = 0;
  uint64_t slot_total = 0, slot_max = 0; // bytes of all slots, of the largest
};
// hsrans_encode_device_ex's refusals, in its order, and its routes; *job gets the arguments as the chain takes them
ExRoute ex_route(int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity, const hsrans_encode_opts *opts, ChainJob *job);
// the summaries request: job->unit, job->n_units; false: more units than a launch has workgroups
bool chain_units(ChainJob *job);
EncParams chain_units_params(const ChainJob &job); // what the summary kernels read: S, bits, in, n, block = unit, n_blocks = n_units
// the host walk over the summaries that came down (reference_blocks / fixed_blocks): job->spans
bool chain_walk(ChainJob *job, const UnitSummary *units);
// the ChainBlocks, the counts and the interval / listed checkpoint bookkeeping from job->spans
void chain_prepare(ChainJob *job);
// A prepared job's device memory.  up (host -> device): blocks, counts, listed checkpoints.  down (device -> host): image sizes, image offsets,
// result words.  ck: checkpoint states, checkpoint positions and, with a plan, the block states (offsets in 32-bit words).  Regions are 256-byte aligned.
struct ChainUp
{
  size_t blocks, counts, list, bytes;
};
struct ChainDown
{
  size_t image_bytes, image_off, result, bytes;
};
struct ChainCk
{
  size_t ck_pos, block_states, bytes;
};
ChainUp chain_up_layout(const ChainJob &job);
ChainDown chain_down_layout(const ChainJob &job);
ChainCk chain_ck_layout(const ChainJob &job);
inline size_t chain_up_bytes(const ChainJob &job) { return chain_up_layout(job).bytes; }
inline size_t chain_down_bytes(const ChainJob &job) { return chain_down_layout(job).bytes; }
inline size_t chain_ck_bytes(const ChainJob &job) { return chain_ck_layout(job).bytes; }
void chain_up_fill(const ChainJob &job, uint8_t *host_up); // the up region's content
// the coding wavefront's and the gather's parameters, the job's regions at the given device addresses
EncParams chain_params(const ChainJob &job, uint8_t *d_scratch, uint8_t *d_down, uint8_t *d_up, uint8_t *d_ck);
// the plan's size, known once the job is prepared
size_t chain_plan_bytes(const ChainJob &job);
// the plan finish: the device's block and checkpoint records through the host encoder's plan assembly; the plan's size, 0: it does not fit
size_t chain_plan_finish(const ChainJob &job, uint64_t total, const uint64_t *image_bytes, const uint64_t *image_off, const uint32_t *block_states,
                         const uint32_t *ck_states, const uint32_t *ck_pos, uint8_t *plan_out, size_t plan_capacity);

// ---- what the host-ranges gathers share (hsrans_capi_gather.cpp): hsrans_decode_device_gather and hsrans_decode_device_gather_batch ----
// the segment length L a gather of d cuts its ranges at: hsrans_gather_segment's rule with the plan's floor (HSRANS_GATHER_MIN_SEGMENT
// when the plan was made, else the compiled-in one)
uint64_t gather_segment_of(const hsrans_dplan *d);
// whether d can be gathered from over a stream of stream_length bytes: it has entry points (no walk plan, at least one chain) and is that stream's
inline bool gather_plan_ok(const hsrans_dplan *d, size_t stream_length)
{
  return !(d->hdr.flags & hsrans::kPlanWalk) && d->hdr.n_chains != 0 && stream_length == d->hdr.stream_len;
}
// what the gather kernels need of d bound to the stream at d_stream (the table fields are null / 0 for a plan without a host-built table)
inline hsrans::GatherSource gather_source_of(const hsrans_dplan *d, const void *d_stream, size_t stream_length)
{
  return hsrans::GatherSource{d->d_plan, d->d_status, (const uint8_t *)d_stream, stream_length, d->pa.table, d->pa.hist_copy, d->pa.hist_off};
}
// the table layout d's gathers use, as gather_shape takes it: that of its host-built table, 0 where its waves build their own
inline uint32_t gather_table_mode(const hsrans_dplan *d) { return d->pa.table != nullptr ? d->pa.table_mode : 0; }
// task(begin, end) for every one-wave task of decoded bytes [offset, offset + length): the range cut at the absolute multiples of L (> 0)
template <typename Task>
inline void gather_cut_range(uint64_t offset, uint64_t length, uint64_t L, Task &&task)
{
  const uint64_t stop = offset + length;
  for (uint64_t b = offset; b < stop;)
  {
    const uint64_t cut = (b / L + 1) * L, e = cut < stop ? cut : stop;
    task(b, e);
    b = e;
  }
}
// A region of the context's task buffers (ctx->h_gather, its device twin), under ctx->lock.  The buffers are used as two halves, call
// after call taking the next region: a queued gather's tasks are never overwritten under it.  gather_region_take grows the buffers
// where `need` (a multiple of 256) asks for it and waits for the last launch that used a half before the half is entered again; the
// caller fills `host`, calls gather_region_order, queues the copy to `dev` and its launches on `s`, then gather_region_commit.
struct GatherRegion
{
  uint8_t *host = nullptr, *dev = nullptr;
  uint32_t half = 0;
  size_t bytes = 0;
};
int gather_region_take(hsrans_ctx *ctx, size_t need, GatherRegion *region);
// gathers of one context form one chain on the device, whatever streams they are queued on: `s` waits for the gather before it
int gather_region_order(hsrans_ctx *ctx, hipStream_t s);
// records the region's event behind the launches on `s` and moves the cursor; HSRANS_E_HIP: nothing is recorded, the region is free again
int gather_region_commit(hsrans_ctx *ctx, const GatherRegion &region, hipStream_t s);
// The whole protocol for a list of `bytes` bytes that one launch (or one chain of launches that fails as a whole) reads: take a region of
// up256(bytes), fill(host pointer) -> HSRANS_* writes the list, order, one stream-ordered copy, launch(device pointer) -> hipError_t,
// commit.  The caller holds ctx->lock and has set the device.  What take, fill and commit return is returned as it is; a failed order,
// copy or launch gives HSRANS_E_HIP, the last two with HIP's error cleared and nothing committed: the region is free again.
template <typename Fill, typename Launch>
inline int gather_region_upload(hsrans_ctx *ctx, size_t bytes, hipStream_t s, Fill &&fill, Launch &&launch)
{
  GatherRegion region;
  int rc = gather_region_take(ctx, up256(bytes), &region);
  if (rc != HSRANS_OK || (rc = fill(region.host)) != HSRANS_OK)
    return rc;
  if (gather_region_order(ctx, s) != HSRANS_OK)
    return HSRANS_E_HIP;
  if (hipMemcpyAsync(region.dev, region.host, bytes, hipMemcpyHostToDevice, s) != hipSuccess || launch(region.dev) != hipSuccess)
  {
    (void)hipGetLastError();
    return HSRANS_E_HIP;
  }
  return gather_region_commit(ctx, region, s);
}

// The status word of an object whose indirect calls the device can refuse (kStatusBadRange), in device memory: made and zeroed on ctx's
// device; read on `stream`, which is waited for — a word that is set is cleared again and reported as HSRANS_E_DEVICE (the caller has set
// the device).  hsrans_capi_gather_batch.cpp; hidden: the library's list of exported symbols stays as it was.
__attribute__((visibility("hidden"))) int refusal_word_create(hsrans_ctx *ctx, uint32_t **word);
__attribute__((visibility("hidden"))) int refusal_word_take(uint32_t *word, hipStream_t stream);

// ---- what the first decodes share (hsrans_capi_index.cpp): hsrans_decode_device_indexing and hsrans_decode_device_indexing_batch ----
// What a recording pass writes besides the output: checkpoint states and read cursors, and for a block_ walk the block records, the states
// on entry to each block and the block count.  Byte counts of the first four.
struct PassBytes
{
  size_t st, wd, blk, bst;
  size_t all() const { return st + wd + blk + bst; }
};
struct PassBuffers // device
{
  uint32_t *ck_states;
  uint64_t *ck_words;
  uint64_t *walk_blocks; // null: not a walk
  uint32_t *walk_states, *walk_count;
  uint32_t max_blocks;
};
inline PassBytes pass_bytes(uint64_t n_ck, uint32_t S, uint64_t max_blocks) { return {(size_t)n_ck * S * 4, (size_t)n_ck * 8, (size_t)max_blocks * 24, (size_t)max_blocks * S * 4}; }
// room for blocks of >= 4 KiB on average (the reference's smallest block is 32 KiB, block_rANS32x64_16w_encode.cpp:21-39); a stream with more gets no plan
inline uint64_t walk_max_blocks(uint64_t decoded_len) { return decoded_len / 4096 + 16; }
// the checkpoints a pass over decoded_len bytes at `interval` groups has room for
inline uint64_t pass_checkpoints(uint64_t decoded_len, uint32_t S, uint32_t interval) { return decoded_len / S / interval + 2; }

// The argument checks of a first decode (the single call's, and every member's of the batch): HSRANS_OK, HSRANS_E_ARG or HSRANS_E_FORMAT.
// base plans only: one single-piece chain per block (raw: one chain), or a block_ stream's walk plan (one chain that follows the inline headers)
inline int indexing_args_check(const hsrans_ctx *ctx, const hsrans_dplan *d, const void *d_stream, size_t stream_length, const void *d_out, size_t out_capacity,
                               uint32_t index_interval)
{
  if (ctx == nullptr || d == nullptr || d_stream == nullptr || d_out == nullptr || d->ctx != ctx)
    return HSRANS_E_ARG;
  if (((uintptr_t)d_stream & 15) != 0 || ((uintptr_t)d_out & 3) != 0 || index_interval == 0 || (index_interval % 4) != 0)
    return HSRANS_E_ARG;
  const PlanHeader &h = d->hdr;
  const bool walk = (h.flags & kPlanWalk) != 0;
  if (h.n_pieces != h.n_chains || h.interval != 0 || d->d_plan == nullptr || d->plan_bytes == 0 || (walk && (h.container != HSRANS_BLOCK || h.n_chains != 1)))
    return HSRANS_E_ARG;
  if (stream_length < h.stream_len || out_capacity < h.decoded_len)
    return HSRANS_E_FORMAT;
  return HSRANS_OK;
}
// whether the first decode with base plan h is assembled on the device behind an mt_ recording pass (else: a walk plan's, or on the host)
inline bool indexing_mt_on_device(const PlanHeader &h) { return h.container == HSRANS_MT && (h.flags & (kPlanWalk | kPlanHasHist | kPlanMergeable)) == 0; }

// The plan a device assembly writes, with room for max_chains chains and max_groups groups.  Its arena's scratch: the assembly's IndexResult
// (and at +128 a walk's block count), from +256 `off_words` chain / group offsets, behind them (16-byte aligned) `extra` bytes.  null: no memory
constexpr size_t kAssemblyCount = 128, kAssemblyOffsets = 256;
hsrans_dplan *assembly_plan(hsrans_ctx *ctx, uint32_t S, uint32_t max_chains, size_t max_groups, size_t off_words, size_t extra, hipStream_t s, uint8_t **scratch);
// The sizes of a block_ member's first decode, from its walk plan's header and the interval; false: more chains than a plan holds
struct WalkAssemblySizes
{
  uint64_t n_ck, max_blocks, max_chains, max_groups;
  PassBytes pbytes;
};
bool walk_assembly_sizes(const PlanHeader &h, uint32_t interval, WalkAssemblySizes *z);
// ... its pass buffers in the new plan's scratch (the checkpoints are the caller's) and the arguments of its assembly kernels
void walk_assembly_args(const hsrans_ctx *ctx, const hsrans_dplan *d, const hsrans_dplan *nd, uint8_t *scratch, uint32_t interval, const WalkAssemblySizes &z, PassBuffers *pass,
                        WalkIndexArgs *wa);
// The sizes and the arguments of an mt_ member's (indexing_mt_on_device)
struct MtAssemblySizes
{
  uint64_t n_ck;
  uint32_t max_chains, max_groups;
  PassBytes pbytes;
};
MtAssemblySizes mt_assembly_sizes(const hsrans_ctx *ctx, const PlanHeader &h, uint32_t interval);
void mt_assembly_args(const hsrans_ctx *ctx, const hsrans_dplan *d, const hsrans_dplan *nd, uint8_t *scratch, uint32_t interval, const MtAssemblySizes &z, const PassBuffers &pass, IndexArgs *ia);
// finish_assembly in two halves, to run around one synchronisation of `s`.  Behind the pass and the assembly kernels: the copy down of what the
// count kernel left and of the base plan d's status word is queued (false: the runtime refused) ...
bool assembly_copy_down(const hsrans_dplan *d, const IndexResult *d_result, hipStream_t s, IndexResult *r, uint32_t *status);
// ... and once `s` is synchronised: rc is what the pass and the copies came to (HSRANS_OK, or why there is no plan); the result is checked
// against the bounds and nd takes over the plan the device wrote (host_groups: as dplan_adopt).  On failure nd is destroyed.
int assembly_adopt(const hsrans_dplan *d, hsrans_dplan *nd, int rc, const IndexResult &r, uint32_t interval, uint32_t min_chains, uint32_t max_chains, uint32_t max_groups,
                   hipStream_t s, const Group *host_groups = nullptr);

// a page-locked, device-mapped host range: the address the GPU reaches it at, else null (hsrans_capi.cpp)
uint8_t *device_view_of_host(const void *ptr, size_t bytes);
// hsrans_decode_device_indexing's body; have_lock: the caller holds ctx->lock already (hsrans_capi_index.cpp)
int decode_device_indexing_impl(hsrans_ctx *ctx, hsrans_dplan *d, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                                uint32_t index_interval, void *hip_stream, hsrans_dplan **indexed, bool have_lock);

#endif // HSRANS_INTERNAL_H
