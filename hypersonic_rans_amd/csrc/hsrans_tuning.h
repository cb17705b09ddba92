// hsrans_tuning.h — every HSRANS_* tuning, comparison and diagnostics switch of the library as one value (host only).
// read_tuning() is the one reader of the environment.  The objects that launch take a copy when they are made: a context at
// hsrans_ctx_create, a device plan at every (re)fill, a batch, a sharded decode and a host pipeline at their create calls.  Nothing is read
// at a launch, and no tuning state is shared between threads.  (HSRANS_DEVICE, the drop-in entries' device, and HSRANS_CPU_WIDE_MODE, the
// host decoder's table layout, are read where they are used: neither has a context.)  The defaults are the measured best.
#ifndef HSRANS_TUNING_H
#define HSRANS_TUNING_H

#include <stdint.h>

namespace hsrans
{

// The domain of a list of class lengths (the nine HSRANS_*_WEIGHTS lists of 8 per-mille values, HSRANS_DEALT_WEIGHTS and
// HSRANS_BATCH_WEIGHTS): eight values, EVERY one of them kClassLengthMin .. kClassLengthMax as written — the bounds the suite holds
// hsrans_ctx_calibrate's fits to (tests/test_gpu_calibrate.py; its lengths always sum to 8000, so no fit can wrap a table).  read_tuning
// ignores any other list as a whole (as it ignores a list of fewer than eight values): the defaults stay, nothing is clamped or
// reshaped.  The nine lists are then rescaled to a sum of at most 8000 (33 .. 6486 a class), the two others
// are taken as written.  What the launches need of a list and the domain gives them (tests/test_geometry_domain.py holds a model of every
// share rule to it):
//   - a class of at least 10 in each half, so that no cumulative table (w / 10 per wave: class_cum_of, hsrans_launch.cpp) ends in 0.
//     With a zero half k_decode_grouped's weighted split gives every wave of the grid's second half the share [0, 0) of its block — the
//     block is never decoded — and k_decode_dealt divides by the table's last entry.  A zero CLASS beside live ones is safe in every
//     kernel (a wave whose share is empty skips its run: `first >= last` in run_grouped, run_spread's `while (i < last)`, `have` in
//     run_dealt, a run_len of 0 in run_persistent), but the domain keeps it out as well: one rule for all eight values;
//   - a table that fits its uint16_t entries: 16 waves x 3000 / 10 = 4800 at the most (unbounded values wrapped it, and the kernel's wave
//     shares were no longer the ones deal_shares had dealt);
//   - a sum of at most 8000 where static shares are cut (static_shares: static_total <= n_chains).
constexpr uint32_t kClassLengthMin = 100, kClassLengthMax = 3000;

struct Tuning
{
  uint32_t waves_per_wg = 16;    // HSRANS_WAVES_PER_WG (4-16): waves per workgroup of the shared-table launches
  bool waves_per_wg_set = false; // ... set at all (any value): grouped launches keep it instead of four 8-wave workgroups per CU
  bool spread = true;            // HSRANS_SPREAD=0: grouped plans with few large blocks keep the one-block-per-workgroup launch
  // HSRANS_SLOT_WEIGHTS: per-mille run length of the 8 wave classes, see PersistentArgs::run_len.  Measured on
  // MI355X at 8 waves per SIMD (bits <= 12): with equal runs the four age classes of a workgroup finish at 33/36/39/42 us,
  // with these weights all at 39 us (tools/stamps.py), 3-7 % less kernel time; at 4 waves per SIMD (bits >= 13) equal
  // runs are better and are kept.
  uint32_t slot_weights[8] = {1328, 1268, 1211, 1145, 1018, 875, 665, 490}; // (re-fitted after the wait fix; runs are whole chains, so this fit is coarse)
  // HSRANS_SLOT_WEIGHTS4: the same for launches with one 16-wave workgroup per CU (4 waves per SIMD: 13-bit tables)
  uint32_t slot_weights4[8] = {1150, 1050, 950, 850, 1150, 1050, 950, 850};
  // HSRANS_DIRECT_WEIGHTS / HSRANS_DIRECT_WEIGHTS4: the chain lengths of the one-chain-per-wave index (hsrans_index_boundaries),
  // per mille of the mean, by the same 8 classes.  Here nothing evens out a wrong weight afterwards (the queues above only hold the
  // short tail chains), so these are fitted until all classes finish together (tools/tune_weights.py: the spread of the classes'
  // mean finish times goes from 19.8 us with the weights above to 0.1 us): the waves of a CU's first workgroup run ahead of
  // the second one's on every SIMD, and inside a workgroup the older waves a little ahead of the younger.
  // One set per occupancy (waves per SIMD): 8 = two 16-wave workgroups per CU (bits <= 12), 6 = two 12-wave workgroups (15 bits,
  // rank table), 4 = one 16-wave workgroup (13 bits), 3 = one 12-wave workgroup (14 bits).
  // (Re-fitted after the decode loops stopped draining the memory queue every iteration: the oldest class now runs three times as
  // many groups as the youngest in the same time.  The same fit with the buffers rotated through HBM lands within 2 % of these.)
  uint32_t direct_weights[8] = {1396, 1332, 1244, 1131, 960, 809, 643, 484}; // (round 3, after the loop's scalar bookkeeping was trimmed: between the fits of two boxes; hsrans_ctx_calibrate fits them to the device at hand)
  bool direct_weights_set = false; // HSRANS_DIRECT_WEIGHTS set to a list inside the domain: it rules over the calibrated sets (direct_weights_for)
  uint32_t direct_weights6[8] = {1192, 1159, 1120, 1072, 976, 907, 829, 745};
  uint32_t direct_weights4[8] = {1097, 1053, 977, 873, 1098, 1053, 977, 873};
  uint32_t direct_weights3[8] = {1052, 1025, 986, 936, 1052, 1025, 986, 936};
  // 32-state plans (two chains per wave, one per half: run_direct_pair, hand-scheduled pair loop; HSRANS_DIRECT_WEIGHTS_PAIR): with 7
  // scalar instructions per group the CU's scalar unit is contended and the oldest waves get nearly all of it
  uint32_t direct_weights_pair[8] = {1662, 1550, 1365, 1142, 887, 656, 450, 289}; // (re-fitted twice in round 3 as the pair loop lost scalar instructions: 1847 ... 204 before)
  // HSRANS_PRIVATE_PAIR: 0 = never, 1 = when there are more chains than wave slots (default), 2 = always pair the
  // chains of 32-state plans in private-table launches.  Measured: 2^30 B in 16,384 blocks 1.40 -> 1.33 ms, but 100 MB in 1,526
  // blocks 0.25 -> 0.30 ms (everything is latency-bound there and half as many waves are in flight)
  uint32_t private_pair = 1;
  uint32_t single_fast = 1; // HSRANS_SINGLE_FAST: 0 = un-indexed raw streams on the general kernel (one wave, two LDS round trips per group)
  uint32_t dual = 1;        // HSRANS_DUAL: 0 = never run two chains per wave (k_decode_dual), 1 = where it pays (default), 2 = for every width (experiment)
  // HSRANS_DUAL_WEIGHTS[_WIDE]: the one-chain-per-wave weights of the dual kernel's launches (one 16-wave workgroup per CU, two chains per wave)
  uint32_t dual_weights[8] = {1232, 1112, 934, 722, 1232, 1112, 934, 722};      // 13 bits (8-byte table)
  uint32_t dual_weights_wide[8] = {1160, 1077, 955, 810, 1160, 1077, 955, 810}; // 14 / 15 bits (rank table; fitted with 4 pairs rotated: spread of the classes' finish 5.4 -> 0.2 us)
  // HSRANS_TABLE_SPILL=1: host-built tables stay in global memory (kModeSpill, BASELINE config 3's comparison side); read per device plan,
  // so that one process can time both sides on the same buffers (bench.py's config-3 leg)
  bool table_spill = false;
  // HSRANS_GROUP_PRIO: per mille of a run decoded at raised priority (measured at 2^30 bytes, two runs each on one box: 0 -> 0.447-0.450 ms,
  // 300 -> 0.440, 500 -> 0.440-0.445, 700 -> 0.447-0.451, 1000 -> 0.452-0.455)
  uint32_t group_prio = 350;
  uint16_t group_prio_class[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFFFF}; // HSRANS_GROUP_PRIO_CLASS: ten per-mille values, see KParams::group_prio_class (tools/group_prio_probe.py)
  bool group_static = false; // HSRANS_GROUP_STATIC: grouped launches hand their groups out in list order, no ticket counter (comparison)
  uint32_t dealt = 1;        // HSRANS_DEALT=0: grouped plans keep k_decode_spread / k_decode_grouped (comparison)
  bool dealt_wide = true;    // HSRANS_DEALT_WIDE=0: 13 / 14 bits keep the grouped launch (comparison)
  uint32_t dealt_min_chains = 1400; // HSRANS_DEALT_MIN_CHAINS: chains per 1,000 waves of the launch below which a plan is not dealt (tuning; 100 MB in 256 KiB blocks, G = 128 — 1.49 chains a wave — 58.5 us grouped, 47.4 dealt; one chain a wave leaves the class weights nothing to work with)
  uint32_t dealt_weights[8] = {};   // HSRANS_DEALT_WEIGHTS: 8 per-mille class lengths of the dealt launch (inside the domain above, as written), where set
  bool dealt_weights_set = false;
  uint32_t dealt_wt = 1;            // HSRANS_DEALT_WT=0: k_decode_dealt's stores as `nt` instead of written through (comparison)
  uint64_t dealt_gap_groups = 17;   // HSRANS_DEALT_GAP_GROUPS: a second prologue is ~2.5 us = ~17 groups of decoding at 8 waves per SIMD (tuning)
  bool dealt_trace = false;         // HSRANS_DEALT_TRACE: why a plan is or is not dealt, on stderr
  uint32_t batch_weights[8] = {}; // HSRANS_BATCH_WEIGHTS: 8 per-mille run lengths of a batch's one-chain-per-wave launch (inside the domain above, as written), where set
  bool batch_weights_set = false;
  bool batch_stamps = false;          // HSRANS_BATCH_STAMPS: per-wave finish times of a batch's first shared launch
  bool shard_one_launch = true;       // HSRANS_SHARD_ONE_LAUNCH=0: a launch per sub-run (comparison: tools/shard_projection.py)
  bool calibrate = false;             // HSRANS_CALIBRATE=1: hsrans_ctx_create fits the class lengths to the device right away
  bool hip_strict = false;            // HSRANS_HIP_STRICT=1: a plan-less raw hsrans_decode_host records its checkpoints on the GPU
  bool host_index_cache_off = false;  // HSRANS_HOST_INDEX_CACHE_OFF: hsrans_decode_host keeps no index between calls
  bool index_assemble_on_host = false; // HSRANS_INDEX_ASSEMBLE_ON_HOST: an indexing decode's plan is assembled on the host (round 3's path)
  bool hpipe_direct = false;          // HSRANS_HPIPE_DIRECT: host pipelines store straight into page-locked output
  bool debug_stamps = false;          // HSRANS_DEBUG_STAMPS: per-wave time stamps (diagnostic library) and the encoders' phase times
  bool hpipe_trace = false;           // HSRANS_HPIPE_TRACE: per-slice timeline of a host pipeline on stderr
  bool indexing_trace = false;        // HSRANS_INDEXING_TRACE: phase times of an indexing decode on stderr
  uint32_t gather_min_segment = 0;    // HSRANS_GATHER_MIN_SEGMENT: floor of a gather task's segment in decoded bytes, 64 .. 2^30 (0: kGatherMinSegment; tools/gather_rate.py sweeps it), read per device plan
};

// the switches as the environment sets them now (about 3 us)
Tuning read_tuning();

} // namespace hsrans

#endif // HSRANS_TUNING_H
