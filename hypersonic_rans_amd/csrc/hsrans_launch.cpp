// hsrans_launch.cpp — the decode launch policy: table choice and the host-built rank table, the launch decision (launch_shape, choose_launch),
// shares and class weights, the batch and gather launch shapes.  Host arithmetic only: it names no kernel function, launches nothing and calls
// no HIP runtime function (hipError_t, uint2 and __host__ __device__ come from the header-only part of hip_runtime.h), so it builds with the
// host compiler as plain C++ — in the library by the ordinary .cpp rule, in tools/fuzz and tests/test_launch_policy.py under AddressSanitizer +
// UBSan.  The kernel table, prepare_kernels and every launch_* are in hsrans_kernels.hip; what host and device share is kernels_layout.h.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "hsrans_kernels.h"
#include "hsrans_plan.h"
#include "kernels_layout.h"

namespace hsrans
{

int index_pass_mode(uint32_t bits) { return bits >= 13 ? kModeTwoLevel : bits == 12 ? kModePackM1 : kModePack; }

// rows of wavefronts per member of a fill launch: as many as the member with the most blocks has, as k_walk_index_fill's at most 2,048, and
// no more than 2^20 workgroups in all
uint32_t index_fill_rows(uint32_t n, uint32_t most_blocks)
{
  const uint32_t cap = std::max(1u, std::min(2048u, (1u << 20) / n));
  return std::max(1u, std::min(most_blocks, cap));
}

// the tuning switches are a Tuning (hsrans_tuning.h) that every launch path is handed; the one constant left is exported
static constexpr uint32_t g_pack64_max_bits = 14; // widest histogram decoded with the 8-byte-per-slot shared table (knob removed in round 5: settled)

uint32_t pack64_max_bits() { return g_pack64_max_bits; }

// Which host-built decode table a plan that carries its histogram gets, and whether its launch runs two chains per wave.
// `direct`: the plan has one chain per wave (PlanHeader::interval == 0), which is what the dual kernel is written for.
TableChoice choose_table(const Tuning &tn, uint32_t bits, uint32_t states, bool direct)
{
  TableChoice t{0, false};
  if (tn.table_spill)
    t.mode = kModeSpill;
  else if (direct && tn.dual == 2 && states == 64 && bits <= 12) // experiment: the dual kernel below 13 bits too
  {
    t.mode = kModePack64;
    t.dual = true;
  }
  else if (direct && tn.dual && states == 64 && bits >= 13)
  {
    // one workgroup of 16 waves per CU, two chains per wave: 13 bits keeps the 8-byte-per-slot table (64 KiB + 32 rings = 144 KiB);
    // at 14 / 15 bits that table does not fit beside 32 rings, so the rank table (18 / 34 KiB).  Measured (100 MB, last wave
    // done, fitted weights, hand-scheduled loops): 13 bits 42.7 us against 49.7 us one chain per wave; 14 / 15 bits 52.3 / 52.7 us
    // (round 2's coarse + fine tables: 57.8 / 57.7; one chain per wave beside the 128 KiB one-lookup table at 14 bits: 63.3)
    t.mode = bits == 13 ? kModePack64 : kModeRank;
    t.dual = true;
  }
  else if (bits <= g_pack64_max_bits && bits != 14) // (wide histograms take the rank table: 52 against 57-63 us, CHANGELOG round 2-3)
    t.mode = kModePack64;
  else if (bits >= 13)
    t.mode = kModeRank; // (14 bits too: beside the 128 KiB one-lookup table only 12 waves fit a CU — 0.31 against 0.37 with a checkpoint every 32 groups)
  return t;
}

size_t rank_table_entries(uint32_t bits) { return table_bytes_for(kModeRank, bits) / 8; }

size_t build_rank_table(const uint16_t counts[256], uint32_t bits, uint2 *out, size_t capacity_entries)
{
  if (bits < 13 || bits > 15 || capacity_entries < rank_table_entries(bits))
    return 0;
  // the 32 most frequent symbols — nearly every lane of a group — get 32 different bank pairs of the entry table (indexed by
  // symbol value, symbols 32 apart would share banks: 8.0 instead of 7.3 bank-conflict cycles per group)
  uint8_t *rank_of_slot = (uint8_t *)out;
  uint2 *ent = (uint2 *)(rank_of_slot + (1u << bits));
  uint32_t order[256];
  for (uint32_t s = 0; s < 256; s++)
    order[s] = s;
  std::stable_sort(order, order + 256, [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
  uint8_t rank[256];
  for (uint32_t r = 0; r < 256; r++)
    rank[order[r]] = (uint8_t)r;
  uint32_t cumul = 0;
  for (uint32_t s = 0; s < 256; s++)
  {
    ent[rank[s]] = make_uint2((uint32_t)counts[s] | (s << 24), 0u - cumul);
    for (uint32_t k = 0; k < counts[s] && cumul + k < (1u << bits); k++)
      rank_of_slot[cumul + k] = rank[s];
    cumul += counts[s];
  }
  return cumul == (1u << bits) ? rank_table_entries(bits) : 0;
}

DeviceGeom default_geom()
{
  DeviceGeom g{};
  g.max_lds = 160 * 1024;
  g.num_cus = 256; // MI355X
  return g;
}

constexpr uint32_t kSpreadWaves = 16;

// (`cum`: the weights the launch will hand the kernel — computed ONCE per launch, so that the check and the kernel cannot see two
// different sets when hsrans_ctx_calibrate rewrites the context's geometry on another thread)
static uint32_t spread_longest_share_of(const DeviceGeom &dg, uint64_t n_chains, const uint16_t (*cum)[17])
{
  const uint32_t grid = spread_grid(dg);
  if (n_chains < (uint64_t)grid * kSpreadWaves || n_chains > (uint64_t)grid * kSpreadMaxShare) // (a chain per wave at least)
    return 0;
  uint32_t longest = 0;
  for (uint32_t b : {0u, (grid + 1) / 2 - 1, (grid + 1) / 2, grid - 1}) // (shares differ by rounding only within a half)
  {
    const uint32_t len = spread_share_begin((uint32_t)n_chains, b + 1, grid, cum[0][kSpreadWaves], cum[1][kSpreadWaves]) -
                         spread_share_begin((uint32_t)n_chains, b, grid, cum[0][kSpreadWaves], cum[1][kSpreadWaves]);
    longest = len > longest ? len : longest;
  }
  longest += 1; // (rounding)
  return longest > kSpreadMaxShare ? 0 : longest;
}

// the class weights of a one-round launch whose waves decode `run_groups` groups each on average: the one-chain-per-wave launch's, this
// device's own once calibrated — the set fitted nearest to that run length where several are (hsrans_ctx_calibrate_runs)
void dealt_weights_now(const Tuning &tn, const DeviceGeom &dg, uint64_t run_groups, uint32_t bits, uint32_t weights_out[8])
{
  direct_weights_for(tn, dg, run_groups, weights_out);
  // 13 / 14 bits (k_decode_dealt_rank): the rank loop's three dependent LDS reads per group make a wave's age count for less — the flatter
  // class lengths fitted for the rank-table one-chain-per-wave launch (Tuning::direct_weights6); nothing calibrates this loop per device.
  // 100 MB in 256 KiB blocks, G = 16, rotated: 14 bits 54.1 us with the 11-bit loop's lengths, 51.3-52.1 with these; 13 bits 52.1 -> 50.0
  // (tools/dealt_weights_probe.py)
  if (bits >= 13)
    for (uint32_t k = 0; k < 8; k++)
      weights_out[k] = tn.direct_weights6[k];
  if (tn.dealt_weights_set) // (HSRANS_DEALT_WEIGHTS: tuning)
    for (uint32_t k = 0; k < 8; k++)
      weights_out[k] = tn.dealt_weights[k];
}

// 8 class weights as the cumulative table the waves of a workgroup of `waves` waves take their parts by: cum[half of the grid][wave].  The
// per-wave shares of a group's chains (run_grouped: kp.group_cum), of a workgroup's share (k_decode_spread, k_decode_dealt: 16 waves)
static void class_cum_of(const uint32_t w8[8], uint32_t waves, uint16_t (*cum_out)[17])
{
  for (uint32_t hf = 0; hf < 2; hf++)
  {
    uint32_t cum = 0;
    for (uint32_t k = 0; k <= 16; k++)
    {
      cum_out[hf][k] = (uint16_t)cum;
      cum += k < waves ? w8[wave_class(hf != 0, k, waves)] / 10 : 0;
    }
  }
}

bool deal_shares(const Tuning &tn, const DeviceGeom &dg, const uint32_t *block_begin, uint32_t n_blocks, uint32_t n_chains, uint64_t total_groups, uint32_t bits, DealtTable *out,
                 uint32_t weights_out[8])
{
  dealt_weights_now(tn, dg, total_groups / ((uint64_t)spread_grid(dg) * kSpreadWaves), bits, weights_out);
  const uint32_t grid = spread_grid(dg);
  if (!tn.dealt || !tn.spread || grid > kDealtGridMax || n_blocks == 0 || block_begin[0] != 0 || block_begin[n_blocks] != n_chains)
    return false;
  if ((uint64_t)n_chains * 1000 < (uint64_t)grid * kSpreadWaves * tn.dealt_min_chains)
    return false;
  // a block and more for every 8-wave workgroup slot of the grouped launch (four per CU): that launch's home ground — one block per slot and
  // round, blocks behind the first round by ticket (256 MiB in 256 KiB blocks: 107-112 us grouped, 119-121 dealt with shares cut at two blocks)
  if (n_blocks >= 2 * grid)
    return false;
  // a workgroup's weight = the sum of its waves' (four waves per class; as the kernel's cumulative table has them); the first half of the grid is resident first
  uint64_t w1 = 0, w2 = 0;
  for (uint32_t k = 0; k < 4; k++)
    w1 += weights_out[k] / 10, w2 += weights_out[4 + k] / 10;
  const uint32_t fh = (grid + 1) / 2;
  uint64_t weight_left = (uint64_t)fh * w1 + (uint64_t)(grid - fh) * w2;
  uint32_t blk = 0; // block of the next share's first chain
  out->begin[0] = 0;
  for (uint32_t b = 0; b < grid; b++)
  {
    // what is left, by the weights that are left: a share that was cut back at a third block leaves its chains to ALL the workgroups behind
    // it (given to the next one alone — targets as fixed fractions of the whole — shares of one grid half ranged from 1.0 to 1.5 blocks
    // at 128 MiB in 256 KiB blocks, and the launch ended 10 us after its median wave: tools/stamps_dealt.py)
    const uint32_t c0 = out->begin[b];
    const uint64_t wb = b < fh ? w1 : w2;
    uint32_t e = b + 1 == grid ? n_chains : c0 + (uint32_t)(((uint64_t)(n_chains - c0) * wb + weight_left / 2) / weight_left);
    weight_left -= wb;
    e = e > n_chains ? n_chains : e;
    while (blk + 1 < n_blocks && block_begin[blk + 1] <= c0) // the block chain c0 is in
      blk++;
    uint32_t split = 0xFFFF;
    if (c0 < n_chains)
    {
      const uint32_t end_a = block_begin[blk + 1];                                   // first block ends here
      const uint32_t end_b = blk + 2 <= n_blocks ? block_begin[blk + 2] : n_chains; // the second one here: the share may not go on
      e = e > end_b ? end_b : e;
      if (e > end_a)
      {
        if (end_a - c0 > 0xFFFE)
          return false;
        split = end_a - c0;
      }
    }
    if (e - c0 > 0xFFFE)
      return false;
    out->begin[b + 1] = e;
    out->split[b] = (uint16_t)split;
  }
  for (uint32_t b = grid; b < kDealtGridMax; b++)
    out->begin[b + 1] = n_chains, out->split[b] = 0xFFFF;
  if (out->begin[grid] != n_chains) // the cuts at third blocks left chains over — blocks much shorter than a share: the grouped launch's case
    return false;
  // ... and where the cuts bent the shares too far from the weights (shares of about two blocks and more), the launch would end with its
  // most loaded workgroup: the grouped launch's case as well
  const double mean = (double)n_chains / (double)((uint64_t)fh * w1 + (uint64_t)(grid - fh) * w2);
  for (uint32_t b = 0; b < grid; b++)
    if ((double)(out->begin[b + 1] - out->begin[b]) / (double)(b < fh ? w1 : w2) > 1.25 * mean + 1.0 / (double)w2)
      return false;
  return true;
}

// Everything about a launch that follows from the plan header and the device alone (no pointers): the table layout, the
// workgroup shape and the grid.  choose_launch starts from it; direct_boundaries uses it to size one chain per resident wave.
LaunchShape launch_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f)
{
  const bool persistent = f.persistent, index_pass = f.index_pass, direct = persistent && f.interval == 0, dual = persistent && f.dual;
  const uint32_t table_mode = persistent ? f.table_mode : 0, n_groups = f.n_groups;
  LaunchShape L{};
  const bool walk = (h.flags & kPlanWalk) != 0;
  const bool grouped = n_groups != 0 && !index_pass;
  L.walk = walk;
  L.shared = !walk && (grouped || (h.shared_hist != 0 && h.n_chains > 1));
  // 64-bit entries only where one table serves a whole workgroup (LDS: 16 KiB table + 16 x 2.25 KiB rings, two per CU)
  const bool rank_table = L.shared && persistent && table_mode == kModeRank;
  const bool spill = L.shared && persistent && table_mode == kModeSpill;
  // (grouped launches from 13 bits on: the rank table, built per block on the device — beside the 64 / 128 KiB one-lookup tables
  // only one workgroup fits a CU: 100 MB in 256 KiB blocks + G=32: 0.269 / 0.206 / 0.190 at 13 / 14 / 15 bits)
  const bool grouped_rank = grouped && h.bits >= 13;
  L.mode = spill ? kModeSpill : rank_table || grouped_rank ? kModeRank : L.shared && h.bits <= pack64_max_bits() ? kModePack64 : h.bits >= 13 ? kModeTwoLevel : h.bits == 12 ? kModePackM1 : kModePack;
  const bool two_level = L.mode == kModeTwoLevel;
  const uint32_t table_bytes = table_bytes_for(L.mode, h.bits);
  const uint32_t wave_bytes = kWaveRingBytes + ((table_bytes + 15) & ~15u); // private rings + table
  uint32_t waves, lds, grid;
  // the LDS of a workgroup of `w` waves around one shared table (lds_layout: the kernels place their pointers by the same rule)
  const auto shared_lds = [&](uint32_t w, uint32_t rings_per_wave = 1, uint32_t extra = 0) { return lds_layout(L.mode, h.bits, w, rings_per_wave, extra).total(); };
  L.dual = dual && L.shared && persistent && (L.mode == kModePack64 || L.mode == kModeRank) && shared_lds(16, 2) <= dg.max_lds;
  if (L.dual)
  {
    // k_decode_dual: workgroups of 16 waves, two rings per wave, wave w decodes chains 2w and 2w + 1 (12 — two workgroups per CU beside a
    // 16 KiB table — measured slower again in round 5: profiles/r05_table_at_zero_ab.txt)
    waves = 16;
    lds = shared_lds(waves, 2);
    const uint32_t per_cu = dg.max_lds / lds ? dg.max_lds / lds : 1;
    L.resident = dg.num_cus * (per_cu * waves > 32 ? 32 / waves : per_cu);
    grid = (h.n_chains + 2 * waves - 1) / (2 * waves);
    if (grid > L.resident)
      grid = L.resident;
  }
  else if (L.shared)
  {
    const uint32_t ring = lds_layout(L.mode, h.bits, 1).ring_stride();
    waves = tn.waves_per_wg;
    // Grouped launches (one workgroup per block, round after round): FOUR workgroups of 8 waves per CU instead of two of 16
    // wherever four fit the LDS.  A round is table build + records + first chunks (~12 us in which the workgroup decodes
    // nothing) and then the decode; with two workgroups per CU the other one is alone on the CU meanwhile, 4 waves per SIMD,
    // which is too few to hide the loop's LDS latency.  With four, three are decoding while one is between rounds, and a round
    // is twice as long for the same fixed cost.  Measured at 2^30 bytes: 256 KiB blocks 0.461 -> 0.492 of 8 TB/s, 64 KiB blocks
    // 0.358 -> 0.427 (1 MiB blocks: unchanged).  HSRANS_WAVES_PER_WG still overrides.
    // (only with at least four groups per CU: fewer, e.g. a 100 MB stream in 256 KiB blocks, fill more wave slots as 16-wave workgroups)
    if (grouped && !tn.waves_per_wg_set && 4 * shared_lds(8, 1, kGroupedExtra) <= dg.max_lds && n_groups >= 4 * dg.num_cus)
      waves = 8;
    if (L.mode == kModeRank && shared_lds(waves) > dg.max_lds / 2)
      waves = 12; // 15 bits: 48 KiB of tables + 12 rings = 75 KiB, two workgroups per CU
    if (shared_lds(waves) > dg.max_lds && shared_lds(4) <= dg.max_lds)
      waves = (dg.max_lds - table_bytes) / ring / 4 * 4; // a big table: as many waves as still fit (multiple of 4: one per SIMD)
    while (waves > 1 && (waves / 2 >= h.n_chains || shared_lds(waves) > dg.max_lds))
      waves /= 2;
    lds = shared_lds(waves, 1, grouped ? kGroupedExtra : 0);
    grid = (h.n_chains + waves - 1) / waves;
    if (grouped)
      grid = n_groups;
    const uint32_t per_cu = dg.max_lds / lds ? dg.max_lds / lds : 1; // workgroups one CU can hold (LDS-limited; 32 waves max)
    L.resident = dg.num_cus * (per_cu * waves > 32 ? 32 / waves : per_cu);
    if ((persistent || grouped) && grid > L.resident)
      grid = L.resident;
  }
  else
  {
    // 32-state plans: two chains per wave, one per half, when two tables fit (run_private_pair); not for the index-build pass
    const bool pair = (tn.private_pair == 2 || (tn.private_pair == 1 && h.n_chains >= 32 * dg.num_cus)) && !walk && h.states == 32 && h.n_chains > 1 &&
                      table_bytes <= 16384 && !index_pass;
    L.private_pair = pair ? 1 : 0;
    const uint32_t wave_lds = pair ? wave_bytes + ((table_bytes + 15) & ~15u) : wave_bytes;
    const uint32_t work = pair ? (h.n_chains + 1) / 2 : h.n_chains;
    waves = walk ? 1 : 4;
    while (waves > 1 && (waves * wave_lds > dg.max_lds / 2 || waves / 2 >= work))
      waves /= 2;
    lds = waves * wave_lds;
    grid = walk ? 1 : (work + waves - 1) / waves;
    L.resident = dg.num_cus * (dg.max_lds / (lds ? lds : 1));
  }
  L.waves = waves;
  L.lds = lds;
  L.grid = grid ? grid : 1;
  // run-length weights of the 8 wave classes (per mille of the mean): class = (workgroup in the grid's second half) * 4 + wave / (waves / 4)
  const bool weighted = (waves == 16 || waves == 12) && !two_level; // (the class weights do not pay in the two-level table mode: measured)
  for (uint32_t k = 0; k < 8; k++)
    L.weights[k] = !weighted ? 1000
                   : L.dual   ? (L.mode == kModeRank ? tn.dual_weights_wide : tn.dual_weights)[k]
                   : direct   ? (L.grid > dg.num_cus ? (waves == 16 ? (h.states == 32 ? tn.direct_weights_pair : dg.have_direct_weights ? dg.direct_weights : tn.direct_weights) : tn.direct_weights6) : (waves == 16 ? tn.direct_weights4 : tn.direct_weights3))[k]
                              : (L.grid > dg.num_cus ? (persistent && !grouped && h.states == 32 ? tn.direct_weights_pair : tn.slot_weights) : tn.slot_weights4)[k];
  return L;
}

void direct_weights_for(const Tuning &tn, const DeviceGeom &dg, uint64_t run_groups, uint32_t out[8])
{
  const uint32_t *base = dg.have_direct_weights ? dg.direct_weights : tn.direct_weights;
  if (dg.n_weight_sets == 0 || run_groups == 0 || tn.direct_weights_set) // (an explicit override rules)
  {
    for (uint32_t k = 0; k < 8; k++)
      out[k] = base[k];
    return;
  }
  const uint32_t n = dg.n_weight_sets < 4 ? dg.n_weight_sets : 4;
  uint32_t hi = 0;
  while (hi < n && dg.set_run[hi] < run_groups)
    hi++;
  if (hi == 0 || hi == n) // outside the fitted lengths: the nearest set
  {
    const uint32_t k0 = hi == 0 ? 0 : n - 1;
    for (uint32_t k = 0; k < 8; k++)
      out[k] = dg.set_weights[k0][k];
    return;
  }
  const double a = log((double)dg.set_run[hi - 1]), b = log((double)dg.set_run[hi]), x = log((double)run_groups);
  const double t = b > a ? (x - a) / (b - a) : 0.0;
  for (uint32_t k = 0; k < 8; k++)
    out[k] = (uint32_t)((1.0 - t) * dg.set_weights[hi - 1][k] + t * dg.set_weights[hi][k] + 0.5);
}

// the header launch_shape is asked with for "the full machine": a plan of (states, bits) that shares one histogram and has chains for every
// wave the device can hold
static PlanHeader full_machine_header(uint32_t states, uint32_t bits)
{
  PlanHeader h{};
  h.states = states;
  h.bits = bits;
  h.shared_hist = 1;
  h.n_chains = 1u << 30; // "many": the full machine
  return h;
}

// Group boundaries that cut `total_groups` whole groups into one chain per wave of the direct launch this device would use
// for a mergeable plan of (states, bits): chain w belongs to wave w, its length follows the wave's class weight.
// Boundaries are multiples of 4 groups (the decode loop stores 4 groups at a time).  Returns the number of chains;
// out[k] = first group of chain k + 1 (k < chains - 1).
size_t direct_boundaries(const Tuning &tn, const DeviceGeom &dg, uint32_t states, uint32_t bits, uint64_t total_groups, uint64_t *out, size_t cap)
{
  const PlanHeader h = full_machine_header(states, bits);
  const TableChoice tc = choose_table(tn, bits, states, true);
  LaunchFacts f;
  f.persistent = true;
  f.table_mode = tc.mode;
  f.dual = tc.dual;
  const LaunchShape L = launch_shape(tn, h, dg, f);
  const uint32_t runs_per_wave = (states == 32 || L.dual) ? 2 : 1;
  const uint64_t W = (uint64_t)L.grid * L.waves;
  uint64_t chains = W * runs_per_wave;
  const uint64_t all_units = total_groups / 4; // boundaries in units of 4 groups
  if (chains > all_units / 8) // a chain is worth its 308 bytes of index and its prologue from about 32 groups on
    chains = all_units / 8 ? all_units / 8 : 1;
  if (chains <= 1)
    return 1;
  if (chains - 1 > cap)
    return 0;
  // cumulative weight up to chain k, then boundaries at units * cum / all
  const uint32_t first_half = (L.grid + 1) / 2;
  // the headline's launch shape (64 states, 8-byte table, two 16-wave workgroups per CU): the lengths fitted for runs of this length
  uint32_t w8[8];
  for (uint32_t k = 0; k < 8; k++)
    w8[k] = L.weights[k];
  if (states == 64 && !L.dual && L.waves == 16 && L.grid > dg.num_cus && L.mode == kModePack64)
    direct_weights_for(tn, dg, total_groups / chains, w8);
  auto weight_of = [&](uint64_t chain) {
    const uint64_t w = chain / runs_per_wave;
    const uint32_t blk = (uint32_t)(w / L.waves), wave_in_wg = (uint32_t)(w % L.waves);
    return (uint64_t)w8[wave_class(blk >= first_half, wave_in_wg, L.waves)];
  };
  uint64_t all = 0;
  for (uint64_t k = 0; k < chains; k++)
    all += weight_of(k);
  uint64_t cum = 0, prev = 0;
  size_t n = 0;
  for (uint64_t k = 0; k + 1 < chains; k++)
  {
    cum += weight_of(k);
    uint64_t b = (uint64_t)((unsigned __int128)all_units * cum / all);
    if (b <= prev)
      b = prev + 1; // every chain gets at least one unit
    if (b >= all_units)
      break;
    out[n++] = b * 4;
    prev = b;
  }
  return n + 1;
}

// The batch launch of 64-state plans with 8-byte tables: the one-chain-per-wave launch's own shape (two 16-wave workgroups per CU,
// LDS = 16 rings + the widest member's table) and its age-class weights (the device's own once calibrated).
BatchShape batch_direct_shape(const Tuning &tn, const DeviceGeom &dg, uint32_t max_bits, uint64_t total_groups, uint32_t states)
{
  const PlanHeader h = full_machine_header(states, max_bits);
  // 13-15 bits (64 states): k_decode_dual's shape — one 16-wave workgroup per CU, two chains per wave, the 8-byte table at 13 bits,
  // the rank table at 14 / 15 — and its class lengths
  const bool wide = states == 64 && max_bits >= 13;
  LaunchFacts f;
  f.persistent = true;
  f.table_mode = wide && max_bits >= 14 ? kModeRank : kModePack64;
  f.dual = wide;
  const LaunchShape L = launch_shape(tn, h, dg, f);
  BatchShape b{};
  b.kind = states == 32 ? kBatchPair : !wide ? kBatchDirect : max_bits >= 14 ? kBatchDualRank : kBatchDualPack;
  b.grid = L.grid;
  b.waves = L.waves;
  b.lds = L.lds;
  b.states = states;
  for (uint32_t k = 0; k < 8; k++)
    b.weights[k] = L.weights[k]; // (32 states: the pair loop's own class lengths, Tuning::direct_weights_pair)
  if (states == 64 && total_groups != 0 && L.waves == 16 && L.grid > dg.num_cus)
    direct_weights_for(tn, dg, total_groups / ((uint64_t)L.grid * L.waves), b.weights);
  if (tn.batch_weights_set) // (HSRANS_BATCH_WEIGHTS: tuning)
    for (uint32_t k = 0; k < 8; k++)
      b.weights[k] = tn.batch_weights[k];
  return b;
}

// The grouped batch launch (64-state members, bits <= 12: the 8-byte table built per group): the shape k_decode_grouped would get for a
// plan with all the members' groups and chains
BatchGroupShape batch_grouped_shape(const Tuning &tn, const DeviceGeom &dg, uint32_t bits, uint32_t n_groups, uint64_t n_chains)
{
  PlanHeader h{};
  h.states = 64;
  h.bits = bits;
  h.n_chains = n_chains > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_chains;
  LaunchFacts f;
  f.n_groups = n_groups;
  const LaunchShape L = launch_shape(tn, h, dg, f);
  BatchGroupShape b{};
  b.grid = L.grid;
  b.waves = L.waves;
  b.lds = L.lds;
  class_cum_of(L.weights, L.waves, b.group_cum);
  return b;
}

static uint32_t dealt_lds(uint32_t bits) // 16 rings + two tables (rank tables from 13 bits on) + 2 KiB
{
  return kSpreadWaves * kFastRingBytes + 2 * table_bytes_for(bits >= 13 ? kModeRank : kModePack64, bits) + 2048;
}

bool dealt_eligible(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f)
{
  return f.n_groups != 0 && f.groups_lean && !f.index_pass && h.states == 64 && (h.bits <= 11 || h.bits == 13 || h.bits == 14) && (h.bits <= 11 || tn.dealt_wide) &&
         h.n_pieces == h.n_chains && 2 * dealt_lds(h.bits) <= dg.max_lds;
}

LaunchFacts launch_facts(const KParams &kp, const PartPlan *parts, const uint32_t *dealt_weights)
{
  LaunchFacts f;
  f.persistent = kp.pa.pieces != nullptr;
  f.table_mode = kp.pa.table != nullptr ? kp.pa.table_mode : 0;
  f.interval = kp.pa.interval;
  f.dual = kp.pa.dual != 0;
  f.n_groups = kp.groups != nullptr ? kp.n_groups : 0;
  f.groups_lean = kp.groups_lean != 0;
  f.spread_min_block = kp.spread;
  f.index_pass = kp.ckpt_interval != 0 || kp.ckpt_groups != nullptr;
  f.single_valid = kp.single.valid != 0;
  f.single_ring_entries = kp.single.ring_entries;
  f.calibrating = kp.finish != nullptr;
  f.tickets = kp.group_tickets != nullptr;
  f.parts = parts != nullptr;
  f.n_parts = parts != nullptr ? parts->n : 0;
  f.dealt = dealt_weights != nullptr;
  if (f.dealt)
    memcpy(f.dealt_weights, dealt_weights, sizeof(f.dealt_weights));
  return f;
}

// a uniform-interval launch's static shares: the chains split over the waves by class weight; what rounding leaves goes through the queues.
// false: shares the kernel cannot address
static bool static_shares(const PlanHeader &h, const LaunchShape &L, uint32_t interval, StaticShares *st)
{
  const uint64_t W = (uint64_t)L.grid * L.waves;
  // 32-state streams: two runs per wave (run_persistent_pair)
  st->static_per_wave = (uint32_t)((uint64_t)h.n_chains / (h.states == 32 ? 2 * W : W));
  const uint32_t first_half = (L.grid + 1) / 2, second_half = L.grid - first_half;
  const uint32_t per_class = waves_per_class(L.waves), classes = L.waves / per_class;
  const uint32_t runs_per_wave = h.states == 32 ? 2 : 1; // run_persistent_pair decodes two runs side by side
  uint32_t longest = 0;
  for (uint32_t hf = 0; hf < 2; hf++)
  {
    uint32_t off = 0;
    for (uint32_t k = 0; k < 4; k++)
    {
      st->run_len[hf * 4 + k] = k < classes ? (uint32_t)((uint64_t)h.n_chains * L.weights[hf * 4 + k] / (1000 * W * runs_per_wave)) : 0;
      st->class_off[hf * 4 + k] = off;
      off += st->run_len[hf * 4 + k] * per_class * runs_per_wave;
      longest = st->run_len[hf * 4 + k] > longest ? st->run_len[hf * 4 + k] : longest;
    }
    st->wg_chains[hf] = off;
  }
  st->half_base[0] = 0;
  st->half_base[1] = first_half * st->wg_chains[0];
  st->static_total = first_half * st->wg_chains[0] + second_half * st->wg_chains[1];
  if (st->static_total > h.n_chains) // weights sum to <= 8000 by construction; belt and braces
    return false;
  // a merged run is read through one 32-bit window of the stream (at most one 16-bit word per symbol)
  return (uint64_t)(longest ? longest : 1) * interval * h.states * 2 < 0xFFFF0000ull;
}

LaunchChoice choose_launch(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f)
{
  LaunchChoice c{};
  c.error = hipSuccess;
  if (f.parts && (f.n_parts == 0 || f.n_parts > kMaxLaunchParts))
  {
    c.error = hipErrorInvalidValue;
    return c;
  }
  if (f.dealt && dealt_eligible(tn, h, dg, f))
  {
    // the host-dealt one-round launch (kernels_dealt.h): 13 / 14 bits with two rank tables, a kernel per width
    const bool rank = h.bits >= 13;
    c.kernel = rank ? KernelId(kKDealtRank + 2 * (h.bits - 13) + (f.parts ? 1 : 0)) : f.parts ? kKDealtParts : tn.dealt_wt ? kKDealt : kKDealtNt;
    c.grid = c.shape.grid = spread_grid(dg);
    c.waves = c.shape.waves = kSpreadWaves;
    c.lds = c.shape.lds = dealt_lds(h.bits);
    c.shape.mode = rank ? kModeRank : kModePack64;
    c.shape.shared = true;
    memcpy(c.shape.weights, f.dealt_weights, sizeof(c.shape.weights));
    c.spread = 2;
    class_cum_of(f.dealt_weights, kSpreadWaves, c.cum); // (the weights the shares were dealt with)
    // a second prologue costs Tuning::dealt_gap_groups groups of decoding
    const uint64_t per_chain = h.interval ? h.interval : h.n_chains ? (uint64_t)h.decoded_len / 64 / h.n_chains : 0; // groups per chain: the index interval (a sliced plan keeps the stream's header)
    c.gap_chains = per_chain ? (uint32_t)((tn.dealt_gap_groups + per_chain / 2) / per_chain) : 0;
    return c;
  }
  const LaunchShape &L = c.shape = launch_shape(tn, h, dg, f);
  const bool grouped = f.n_groups != 0 && !f.index_pass;
  c.grid = L.grid;
  c.waves = L.waves;
  c.lds = L.lds;
  if (grouped)
    class_cum_of(L.weights, L.waves, c.cum);
  if (f.persistent && f.interval != 0 && !static_shares(h, L, f.interval, &c.shares))
  {
    c.error = hipErrorInvalidValue;
    return c;
  }
  if (f.persistent && f.interval == 0)
  {
    // one-chain-per-wave launches: the plan's chains as W runs of consecutive chains (run_direct); 32-state and two-chain launches keep their own dealing
    const uint64_t W = (uint64_t)L.grid * L.waves;
    c.run_chains = h.states == 64 && !L.dual ? (uint32_t)((h.n_chains + W - 1) / W) : 1;
  }
  if (f.single_valid && !f.index_pass && tn.single_fast)
  {
    // one chain of one piece (a raw stream without an index): the two-wave latency kernel
    c.kernel = kKSingle;
    c.shape = LaunchShape{};
    c.shape.mode = kModePack64;
    c.grid = c.shape.grid = 1;
    c.waves = c.shape.waves = 2;
    c.lds = c.shape.lds = (8u << h.bits) + (f.single_ring_entries + kSingleMirror) * 16 + 64;
    return c;
  }
  const bool wide_table = L.mode == kModePack64 || L.mode == kModeRank; // what k_decode_dual, k_decode_persist and the PARTS kernels are built for
  if (L.dual)
    c.kernel = KernelId(kKDual + (L.mode == kModeRank ? 1 : 0));
  else if (f.persistent && f.interval != 0 && L.shared && wide_table && f.table_mode != 0 && !f.index_pass)
    c.kernel = KernelId(kKPersist + (L.mode == kModeRank ? 1 : 0));
  else if (grouped && L.shared)
  {
    const int m = L.mode == kModeSpill ? kModePack64 : L.mode;
    c.kernel = f.groups_lean && m >= kModeTwoLevel ? KernelId(kKGroupedLean + m - kModeTwoLevel) : KernelId(kKGrouped + m);
  }
  else if (f.persistent && f.interval == 0 && L.shared)
    c.kernel = L.mode == kModePack64 && f.calibrating && h.states == 64 ? kKCalibrate : KernelId(kKDirect + L.mode);
  else
    c.kernel = L.shared || L.mode >= kModePack64 ? KernelId(kKDecodeShared + L.mode) : KernelId(kKDecodePrivate + L.mode);
  // grouped plans with few, large blocks (spread_min_block: the fewest chains of a block, where the host found the plan eligible): every
  // resident workgroup takes its share of ALL chains and builds the one or two tables it needs (kernels_spread.h)
  if (grouped && L.shared && f.spread_min_block != 0 && f.groups_lean && L.mode == kModePack64 && tn.spread)
  {
    uint16_t spread_cum[2][17];
    // k_decode_spread's wave weights: the one-chain-per-wave launch's (the device's own once calibrated); one snapshot, the same weights
    // for the check below and for the kernel
    const uint32_t *const spread_weights = dg.have_direct_weights ? dg.direct_weights : tn.direct_weights;
    class_cum_of(spread_weights, kSpreadWaves, spread_cum);
    const uint32_t longest = spread_longest_share_of(dg, h.n_chains, spread_cum);
    const uint32_t slds = kSpreadWaves * kFastRingBytes + 2 * table_bytes_for(kModePack64, h.bits) + (kSpreadMaxShare + 1) * (uint32_t)sizeof(Piece);
    if (longest != 0 && longest < f.spread_min_block && 2 * slds <= dg.max_lds) // (a share shorter than every block touches at most two)
    {
      c.spread = 1;
      c.kernel = kKSpread;
      c.grid = spread_grid(dg);
      c.waves = kSpreadWaves;
      c.lds = slds;
      memcpy(c.cum, spread_cum, sizeof(c.cum));
      memcpy(c.shape.weights, spread_weights, sizeof(c.shape.weights)); // (launch info: the lengths the table above was made from, not the grouped shape's)
    }
  }
  if (f.parts)
  {
    // a rank's sub-runs in one launch: only the kernels that count their units into the sub-runs (PartArgs)
    if (c.spread)
      c.kernel = KernelId(kKSpread + 1);
    else if (grouped && L.shared && f.groups_lean && wide_table)
      c.kernel = KernelId(kKGroupedParts + L.mode - kModePack64);
    else
      c.error = hipErrorNotSupported;
  }
  c.dynamic_groups = grouped && !c.spread && f.tickets && f.n_groups > L.grid;
  return c;
}

LaunchInfo launch_info_of(const LaunchChoice &c, uint32_t chains)
{
  LaunchInfo info{};
  info.grid = c.grid;
  info.block = c.waves * 64;
  info.lds_bytes = c.lds;
  info.waves_per_block = c.waves;
  info.chains = chains;
  info.shared_table = c.shape.shared;
  info.walk = c.shape.walk;
  info.two_level = c.shape.mode == kModeTwoLevel;
  info.table_mode = (uint32_t)c.shape.mode;
  info.chains_per_wave = c.shape.dual ? 2 : 1;
  for (uint32_t k = 0; k < 8; k++)
    info.class_weights[k] = c.shape.weights[k];
  info.dynamic_groups = c.dynamic_groups ? 1 : 0;
  info.spread = c.spread;
  return info;
}

// waves per workgroup, LDS and grid of g's layout for n_tasks tasks and a table of table_bytes
static void gather_waves(GatherShape &g, const DeviceGeom &dg, uint32_t table_bytes, uint32_t n_tasks)
{
  // a shared table: lds_layout with plain rings (gather_setup); else every wave has a ring and a table of its own
  const auto lds_of = [&](uint32_t w) { return g.shared ? lds_layout_gather(g.mode, table_bytes, w).total() : w * (kWaveRingBytes + ((table_bytes + 15) & ~15u)); };
  // few tasks: smaller workgroups, so that they reach more CUs (a task is one wave's work whatever the workgroup)
  uint32_t waves = g.shared ? 16 : 4;
  while (waves > 1 && (lds_of(waves) > (g.shared ? dg.max_lds : dg.max_lds / 2) || (waves > (g.shared ? 4u : 1u) && (n_tasks + waves - 1) / waves < 2 * dg.num_cus)))
    waves /= 2;
  g.waves = waves;
  g.lds = lds_of(waves);
  g.grid = (n_tasks + waves - 1) / waves;
}

GatherShape gather_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, uint32_t table_mode, uint32_t n_tasks)
{
  GatherShape g{};
  g.shared = table_mode != 0;
  if (g.shared)
    g.mode = (int)table_mode; // what choose_table gave the plan when it was filled
  else
  {
    // the layout launch_shape gives a plan whose waves build their own tables
    PlanHeader hp = h;
    hp.shared_hist = 0;
    hp.flags &= ~kPlanWalk;
    g.mode = launch_shape(tn, hp, dg, LaunchFacts{}).mode;
  }
  gather_waves(g, dg, table_bytes_for(g.mode, h.bits), n_tasks);
  return g;
}

uint32_t gather_table_bytes(int mode, uint32_t bits) { return (table_bytes_for(mode, bits) + 15) & ~15u; }

GatherShape gather_set_shape(const DeviceGeom &dg, int mode, bool shared, uint32_t table_bytes, uint32_t n_tasks)
{
  GatherShape g{};
  g.mode = mode;
  g.shared = shared;
  gather_waves(g, dg, table_bytes, n_tasks);
  return g;
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather_indirect's launch.  Table layout, waves per workgroup and LDS are gather_shape's for the most tasks the
// call can have; the grid is that bound too, capped at the workgroups the device holds at once (LDS and 32 waves per CU: the
// shared-table kernels run 8 waves per SIMD, the others are bound by their LDS), so every workgroup is resident from the start.
// How k_gather_ranges deals the tasks to its waves: a static stride (task t of wave w, workgroup b: w * grid + b, + grid * waves, ...).
// The alternative, a ticket counter in the workspace that k_gather_cut resets, has not been measured yet; the stride is what ships.
// ---------------------------------------------------------------------------------------------------------------
GatherShape gather_ranges_shape(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, uint32_t table_mode, uint32_t max_count, uint64_t dst_capacity, uint64_t segment)
{
  const uint64_t most = (uint64_t)max_count + (segment ? dst_capacity / segment : 0);
  GatherShape g = gather_shape(tn, h, dg, table_mode, (uint32_t)std::min<uint64_t>(most, 0x7FFFFFFFu));
  const uint32_t per_cu = std::max(1u, std::min(g.lds ? dg.max_lds / g.lds : 32u, 32u / g.waves));
  g.grid = std::max(1u, std::min(g.grid, dg.num_cus * per_cu));
  return g;
}

// ---------------------------------------------------------------------------------------------------------------
// hsrans_decode_device_gather_batch_indirect's launches: gather_ranges_shape's reasoning, kind by kind.  A shared kind's workgroup serves
// whole units (`waves` consecutive tasks of one member), so its grid is counted in units: those of the most tasks the kind can have and
// one more per member that can be named, each member's last unit being partly empty.
// ---------------------------------------------------------------------------------------------------------------
GatherShape gather_set_ranges_shape(const DeviceGeom &dg, int mode, bool shared, uint32_t table_bytes, uint32_t max_count, uint64_t dst_capacity, uint64_t min_segment,
                                    uint32_t kind_members)
{
  const uint64_t most = std::min<uint64_t>((uint64_t)max_count + (min_segment ? dst_capacity / min_segment : 0), 0x7FFFFFFFu);
  GatherShape g = gather_set_shape(dg, mode, shared, table_bytes, (uint32_t)most);
  const uint64_t padding = shared ? std::min(kind_members, max_count) : 0;
  const uint32_t per_cu = std::max(1u, std::min(g.lds ? dg.max_lds / g.lds : 32u, 32u / g.waves));
  g.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)g.grid + padding, (uint64_t)dg.num_cus * per_cu));
  return g;
}
} // namespace hsrans
