// The decode launch policy (hsrans_launch.cpp): which table a plan gets, which kernel a launch runs and in what shape, which wave decodes
// which chains.  Host arithmetic only — no kernel, no launch, no HIP runtime call — so the unit builds with a host compiler (tools/fuzz,
// tests/test_launch_policy.py run it under AddressSanitizer + UBSan).  hsrans_kernels.h includes this header; what host and device must
// agree on is in kernels_layout.h.
#ifndef HSRANS_LAUNCH_H
#define HSRANS_LAUNCH_H

#include <hip/hip_runtime.h> // (hipError_t, uint2, __host__ __device__: the header-only part)
#include <stddef.h>
#include <stdint.h>

#include "hsrans_plan.h"
#include "hsrans_tuning.h"

namespace hsrans
{

struct KParams;  // hsrans_kernels.h
struct PartPlan; // hsrans_kernels.h

// k_decode_dealt (kernels_dealt.h): the host-dealt one-round launch of block_/mt_ plans with checkpoints
constexpr uint32_t kDealtGridMax = 512;
struct DealtTable
{
  uint32_t begin[kDealtGridMax + 1]; // chains; begin[grid] = n_chains
  uint16_t split[kDealtGridMax];     // chains of the share that belong to its first block (>= the share's length: one block only)
};

struct BatchGroupShape
{
  uint32_t grid, waves, lds;
  uint16_t group_cum[2][17];
};
BatchGroupShape batch_grouped_shape(const Tuning &tn, const struct DeviceGeom &dg, uint32_t bits, uint32_t n_groups, uint64_t n_chains);

constexpr uint32_t kBatchDirect = 0, kBatchPair = 1, kBatchDualPack = 2, kBatchDualRank = 3; // which kernel a shared launch runs
struct BatchShape
{
  uint32_t grid, waves, lds, states, kind;
  uint32_t weights[8]; // per-mille run lengths of the 8 wave classes (wave_class, kernels_layout.h)
};

struct LaunchInfo
{
  uint32_t grid, block, lds_bytes, waves_per_block, chains, shared_table, walk, two_level, table_mode, chains_per_wave;
  uint32_t class_weights[8]; // the per-mille run lengths of the 8 wave classes this launch was shaped with (LaunchShape::weights)
  uint32_t dynamic_groups;   // grouped launches: groups handed out by the ticket counter (1) or in static order (0)
  uint32_t spread;           // grouped plan launched by k_decode_spread (chains dealt out evenly, two tables per workgroup); 2: by k_decode_dealt (host-dealt shares)
};

// what the launcher needs to know about the device a context lives on
struct DeviceGeom
{
  uint32_t num_cus, max_lds;
  // per-mille chain lengths of the 8 wave classes of the 64-state one-chain-per-wave launch, fitted to THIS device by
  // hsrans_ctx_calibrate (0 = not calibrated: the constants fitted on the development box, g_direct_weights)
  uint32_t have_direct_weights;
  uint32_t direct_weights[8];
  // The same fit at several RUN LENGTHS (mean groups per wave of the launch; ascending): a wave's time is its prologue plus its groups
  // at its class's rate, so the lengths that make all classes finish together depend on how long the runs are — an old wave's
  // head start counts for less in a long run.  hsrans_ctx_calibrate fits the 48 MiB launch (96 groups per wave),
  // hsrans_ctx_calibrate_runs longer ones; direct_weights_for interpolates between the fitted lengths (in log run length).
  uint32_t n_weight_sets;
  uint32_t set_run[4];
  uint32_t set_weights[4][8];
};
// the per-mille chain lengths of the 8 wave classes for a 64-state one-chain-per-wave launch whose runs average run_groups
void direct_weights_for(const Tuning &tn, const DeviceGeom &dg, uint64_t run_groups, uint32_t out[8]);

// the launch all members of a batch of 64-state plans with 8-byte tables (bits <= 12) share; max_bits = the widest member
// (total_groups: all members' groups together — the class weights follow the launch's mean run length; 0 = the default set)
BatchShape batch_direct_shape(const Tuning &tn, const DeviceGeom &dg, uint32_t max_bits, uint64_t total_groups = 0, uint32_t states = 64);

// a launch's shape as it follows from plan header + device (launch_shape)
struct LaunchShape
{
  int mode;         // decode-table layout (kMode* in kernels_layout.h)
  bool shared, walk, dual;
  uint32_t waves, lds, grid, resident, private_pair;
  uint32_t weights[8]; // per-mille run length of the 8 wave classes
};

// What decides a launch besides the plan header, the device and the tuning: scalars only.  launch_facts reads them off a KParams, so
// every caller of launch_decode describes its launch the same way; hsrans_launch_choice takes them as they are (tests, planning).
struct LaunchFacts
{
  bool persistent = false;       // a kPlanMergeable plan: PersistentArgs is filled
  uint32_t table_mode = 0;       // ... its host-built decode table (kMode*); 0: the kernel builds its own
  uint32_t interval = 0;         // ... uniform chains of this many groups; 0: chains of any length, one (run) per wave
  bool dual = false;             // ... two chains per wave (choose_table)
  uint32_t n_groups = 0;         // grouped plan (block_/mt_ with checkpoints): its groups; 0: none
  bool groups_lean = false;      // ... 64 states, every group a mergeable run or fills only
  uint32_t spread_min_block = 0; // ... KParams::spread
  bool index_pass = false;       // the launch records checkpoints (hsrans_capi_index.cpp)
  bool single_valid = false;     // one chain of one rANS piece (SingleArgs::valid)
  uint32_t single_ring_entries = 0;
  bool calibrating = false;      // hsrans_ctx_calibrate's launches: per-wave finish times
  bool tickets = false;          // grouped: the launch has a ticket counter
  bool parts = false;            // a rank's sub-runs in one launch (PartPlan) ...
  uint32_t n_parts = 0;          // ... so many: 1 .. kMaxLaunchParts, anything else is refused
  bool dealt = false;            // the plan has a valid dealing (deal_shares) ...
  uint32_t dealt_weights[8] = {}; // ... made with these class weights
};

// one value per kernel instantiation a single-plan decode launch can run (the table in hsrans_kernels.hip: name + launch)
enum KernelId : uint32_t
{
  kKDecodePrivate,                   // + mode (kModePack .. kModeTwoLevel): k_decode<mode, false>
  kKDecodeShared = kKDecodePrivate + 3, // + mode (kModePack .. kModeSpill): k_decode<mode, true>
  kKDual = kKDecodeShared + 6,       // + 1: the rank table
  kKPersist = kKDual + 2,            // + 1: the rank table
  kKDirect = kKPersist + 2,          // + mode (kModePack .. kModeSpill)
  kKCalibrate = kKDirect + 6,
  kKGrouped,                         // + mode (kModePack .. kModeRank): k_decode_grouped<mode, false>
  kKGroupedLean = kKGrouped + 5,     // + mode - kModeTwoLevel (.. kModeRank): <mode, true>
  kKGroupedParts = kKGroupedLean + 3, // + mode - kModePack64 (.. kModeRank): <mode, true, true>
  kKSpread = kKGroupedParts + 2,     // + 1: PARTS
  kKDealtNt = kKSpread + 2,          // k_decode_dealt<false, false>
  kKDealt,                           // <true, false>
  kKDealtParts,                      // <true, true>
  kKDealtRank,                       // + 2 * (bits - 13) + PARTS: k_decode_dealt_rank<bits, PARTS>
  kKSingle = kKDealtRank + 4,
  kKernelCount
};

// the static shares of a uniform-interval launch (PersistentArgs' fields of the same names)
struct StaticShares
{
  uint32_t static_per_wave, run_len[8], class_off[8], wg_chains[2], half_base[2], static_total;
};

// Which kernel a single-plan launch runs and how: everything launch_decode needs that is not a pointer.
struct LaunchChoice
{
  hipError_t error;      // hipSuccess, or what launch_decode returns without launching anything
  KernelId kernel;
  uint32_t grid, waves, lds; // of the launch (the spread and dealt launches have their own, not the shape's)
  LaunchShape shape;     // (weights: what the launch's shares were sized with — the dealing's for k_decode_dealt)
  uint32_t spread;       // LaunchInfo::spread: 0, 1 = k_decode_spread, 2 = k_decode_dealt
  bool dynamic_groups;   // grouped: groups behind the first round go by ticket
  uint16_t cum[2][17];   // grouped / spread: KParams::group_cum; dealt: DealtParams::cum
  StaticShares shares;   // uniform-interval launches
  uint32_t run_chains;   // one-chain-per-wave launches: PersistentArgs::run_chains
  uint32_t gap_chains;   // dealt: DealtParams::gap_chains
};

// k_decode_spread (kernels_spread.h): G = two 16-wave workgroups per CU; workgroup b's share of the plan's N chains starts at
// spread_share_begin(b): the first half of the grid weighs w1 per workgroup, the second half w2 (the sums of their waves' age-class
// weights).  A share's piece records are kept in LDS: at most kSpreadMaxShare chains.
constexpr uint32_t kSpreadMaxShare = 127;
inline uint32_t spread_grid(const DeviceGeom &dg) { return 2 * dg.num_cus; }
__host__ __device__ inline uint32_t spread_share_begin(uint32_t n_chains, uint32_t b, uint32_t grid, uint32_t w1, uint32_t w2)
{
  const uint32_t fh = (grid + 1) / 2;
  const uint64_t total = (uint64_t)fh * w1 + (uint64_t)(grid - fh) * w2;
  const uint64_t cum = b <= fh ? (uint64_t)b * w1 : (uint64_t)fh * w1 + (uint64_t)(b - fh) * w2;
  return (uint32_t)((uint64_t)n_chains * cum / total);
}

// the layout a recording pass over a plan of `bits` decodes with (launch_shape's rule for private tables)
int index_pass_mode(uint32_t bits);
// rows of wavefronts per member of a fill launch of the batched first decode: as many as the member with the most blocks has, as
// k_walk_index_fill's at most 2,048, and no more than 2^20 workgroups in all
uint32_t index_fill_rows(uint32_t n, uint32_t most_blocks);

struct GatherShape
{
  int mode;    // decode-table layout (kMode*)
  bool shared; // one LDS table per workgroup, copied from the plan's host-built table; else a table per wave, built from the pieces' histograms
  uint32_t waves, lds, grid;
};
// the launch of n_tasks tasks on a plan: table_mode = the plan's host-built table (PersistentArgs::table_mode; 0: it has none).  The table
// layout is the one the plan decodes with: its host-built table's, else what launch_shape gives a plan whose waves build their own.
GatherShape gather_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, uint32_t table_mode, uint32_t n_tasks);
// the launch shape for ranges only the device knows.  The grid is sized from what the host does know — no more tasks can have
// destinations of their own than max_count + dst_capacity / segment — and capped at the waves the device holds at once; the kernel
// strides over the tasks, so a total above either bound still finishes.
GatherShape gather_ranges_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, uint32_t table_mode, uint32_t max_count, uint64_t dst_capacity, uint64_t segment);
// the LDS a decode table of layout `mode` takes at `bits`, rounded up to 16 bytes (0: the layout that stays in global memory)
uint32_t gather_table_bytes(int mode, uint32_t bits);
// the launch of n_tasks tasks of one kind (mode, shared): waves per workgroup and LDS by gather_shape's rule for table_bytes, the kind's
// largest table; the grid is that of n_tasks entries (a launch whose entries are padded is given its own by the caller)
GatherShape gather_set_shape(const DeviceGeom &dg, int mode, bool shared, uint32_t table_bytes, uint32_t n_tasks);
// the launch shape of one kind for ranges only the device knows: layout, waves and LDS are gather_set_shape's for the most tasks the kind
// can have — max_count + dst_capacity / min_segment (the kind's smallest member segment; 0: no member can have a task) have destinations
// of their own, gather_ranges_shape's bound — the shared kinds add one unit of padding per member that can be named; the grid is capped at
// the workgroups the device holds at once, and the kernels loop
GatherShape gather_set_ranges_shape(const DeviceGeom &dg, int mode, bool shared, uint32_t table_bytes, uint32_t max_count, uint64_t dst_capacity, uint64_t min_segment,
                                    uint32_t kind_members);

DeviceGeom default_geom(); // MI355X: 256 CUs, 160 KiB LDS (used where no device is at hand: host-side index sizing)
LaunchShape launch_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f); // (reads persistent, table_mode, interval, dual, n_groups, index_pass)
struct TableChoice
{
  uint32_t mode; // 0: none (the kernel builds its own), else kMode* of the host-built table
  bool dual;     // two chains per wave (k_decode_dual)
};
TableChoice choose_table(const Tuning &tn, uint32_t bits, uint32_t states, bool direct);
// chain boundaries (in groups) of the direct launch: one chain per resident wave, sized by class weight; see hsrans_launch.cpp
size_t direct_boundaries(const Tuning &tn, const DeviceGeom &dg, uint32_t states, uint32_t bits, uint64_t total_groups, uint64_t *out, size_t cap);
// host-side builder of the bits >= 13 rank decode table (layout: kModeRank in kernels_layout.h); returns entries written
size_t build_rank_table(const uint16_t counts[256], uint32_t bits, uint2 *out, size_t capacity_entries);
size_t rank_table_entries(uint32_t bits);
// widest histogram the shared 8-byte-per-slot table (MODE 3) is used for
uint32_t pack64_max_bits();
// A single-plan decode launch is decided in ONE place, choose_launch: a pure function of the tuning, the plan header, the device and the
// LaunchFacts — no pointer, no HIP call, nothing written — that names the kernel (KernelId), its grid, workgroup and LDS, and the scalars
// the kernel's parameters still need.  It is also where the launch is refused: `parts` with n == 0 or n > kMaxLaunchParts and shares a
// uniform-interval launch cannot address are hipErrorInvalidValue, `parts` with a kernel that cannot count them (plans without groups,
// groups that are not lean, tables other than the 8-byte and the rank table) hipErrorNotSupported.
LaunchChoice choose_launch(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f);
// whether k_decode_dealt can take the plan at all (lean grouped, single-piece chains, 64 states, <= 11 bits or 13 / 14 bits with
// Tuning::dealt_wide, no index pass, two workgroups' LDS per CU): choose_launch's test, and dplan_launch's for whether dealing is worth doing
bool dealt_eligible(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f);
LaunchInfo launch_info_of(const LaunchChoice &c, uint32_t chains); // what hsrans_dplan_launch_info reports of the launch
LaunchFacts launch_facts(const KParams &kp, const PartPlan *parts, const uint32_t *dealt_weights /* null: no valid dealing */);
// The dealing of k_decode_dealt: block k = chains [block_begin[k], block_begin[k + 1]) (n_blocks + 1 entries, the last = n_chains), every one a coded
// block of single-piece mergeable chains.  Workgroup shares by age-class weight (the one-chain-per-wave launch's, this device's own once
// calibrated), each cut back where it would reach into a third block.  false: the plan does not suit the launch (too few chains for the
// device's waves, shares that would have to span more than two blocks, a share beyond 65,535 chains).  weights_out: the 8 class weights used
// (the caller's cache key: a calibration changes them).
bool deal_shares(const Tuning &tn, const DeviceGeom &dg, const uint32_t *block_begin, uint32_t n_blocks, uint32_t n_chains, uint64_t total_groups, uint32_t bits, DealtTable *out,
                 uint32_t weights_out[8]);
void dealt_weights_now(const Tuning &tn, const DeviceGeom &dg, uint64_t run_groups, uint32_t bits, uint32_t weights_out[8]); // run_groups: groups per wave of the launch, on average

} // namespace hsrans

#endif // HSRANS_LAUNCH_H
