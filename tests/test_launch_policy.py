"""csrc/hsrans_launch.cpp on its own: the decode launch policy is host arithmetic in a unit that names no kernel, so a stand-alone program,
compiled by the host compiler from hsrans_launch.cpp, hsrans_tuning.cpp and hsrans_batch_deal.cpp, runs it under AddressSanitizer and UBSan
where the host compiler has them (it loads nothing into Python).

The sweep: devices of 1, 8, 80, 255, 256 and 304 CUs with 64 KiB and 160 KiB of LDS (and one calibrated MI355X), 8 .. 15 bits, 32 and 64 states,
plans of 1, 2, 63, 4096, 47104 and 2^20 chains, block lists of 1, 2, 92 and 2 x grid - 1 blocks, under the default class lengths, the four
named lists of tests/test_geometry_domain.py and 32 seeded random lists of its domain (100 .. 3000), each set through every HSRANS_*_WEIGHTS
knob at once.  It calls choose_launch, deal_shares, direct_boundaries, both batch shapes and the four gather shapes and asserts what the
code's own comments promise, nothing more:

  choose_launch      a successful choice has kernel < kKernelCount, grid >= 1, waves >= 1;
  static shares      a uniform-interval launch's static_total <= n_chains;
  deal_shares        a true result has begin non-decreasing, begin[0] == 0, begin[grid] == n_chains, every share <= 0xFFFE;
  direct_boundaries  boundaries are strictly ascending multiples of 4 below total_groups.

The second test keeps the split in place: no kernel, launch or HIP runtime call in hsrans_launch.cpp, none of its functions back in
hsrans_kernels.hip."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
UNITS = ("hsrans_launch.cpp", "hsrans_tuning.cpp", "hsrans_batch_deal.cpp")

PROGRAM = r"""
#include "hsrans_kernels.h"
#include "hsrans_batch.h"
#include "kernels_layout.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

using namespace hsrans;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) // [0, n)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

static const char *const kKnobs[] = {"HSRANS_SLOT_WEIGHTS",   "HSRANS_SLOT_WEIGHTS4",      "HSRANS_DIRECT_WEIGHTS", "HSRANS_DIRECT_WEIGHTS4",   "HSRANS_DIRECT_WEIGHTS6", "HSRANS_DIRECT_WEIGHTS3",
                                     "HSRANS_DIRECT_WEIGHTS_PAIR", "HSRANS_DUAL_WEIGHTS", "HSRANS_DUAL_WEIGHTS_WIDE", "HSRANS_DEALT_WEIGHTS", "HSRANS_BATCH_WEIGHTS"};
static const uint32_t kNamed[4][8] = {{1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000},
                                      {3000, 2000, 1000, 500, 500, 400, 300, 300},
                                      {300, 300, 400, 500, 500, 1000, 2000, 3000},
                                      {100, 100, 100, 3000, 100, 100, 1500, 3000}};
static const uint32_t kChains[] = {1, 2, 63, 4096, 47104, 1u << 20};

static std::string g_where; // the inputs of the call under way: printed with a failure (a sanitizer report names the call itself)
static unsigned long g_choices, g_refused, g_dealt, g_not_dealt, g_indexes, g_shapes;

#define CHECK(cond)                                                                      \
  do                                                                                     \
  {                                                                                      \
    if (!(cond))                                                                         \
    {                                                                                    \
      printf("FAILED %s  at  %s  (line %d)\n", #cond, g_where.c_str(), __LINE__);        \
      exit(1);                                                                           \
    }                                                                                    \
  } while (0)

static Tuning tuning_under(const uint32_t *list) // null: the defaults
{
  for (const char *knob : kKnobs)
  {
    if (list == nullptr)
    {
      unsetenv(knob);
      continue;
    }
    std::string text;
    for (uint32_t k = 0; k < 8; k++)
      text += (k ? "," : "") + std::to_string(list[k]);
    setenv(knob, text.c_str(), 1);
  }
  return read_tuning();
}

static void check_choice(const Tuning &tn, const PlanHeader &h, const DeviceGeom &dg, const LaunchFacts &f, const char *kind)
{
  g_where += std::string(" ") + kind;
  const LaunchChoice c = choose_launch(tn, h, dg, f);
  g_choices++;
  if (c.error != hipSuccess)
    g_refused++;
  else
  {
    CHECK(c.kernel < kKernelCount && c.grid >= 1 && c.waves >= 1);
    if (f.persistent && f.interval != 0)
      CHECK(c.shares.static_total <= h.n_chains);
    const LaunchInfo info = launch_info_of(c, h.n_chains);
    CHECK(info.block == c.waves * 64);
  }
  g_where.resize(g_where.size() - 1 - strlen(kind));
}

static void sweep(const Tuning &tn, const DeviceGeom &dg, const char *list_name)
{
  const uint32_t grid = spread_grid(dg);
  const uint32_t block_counts[] = {1, 2, 92, 2 * grid - 1};
  std::unique_ptr<DealtTable> table(new DealtTable); // (on the heap, so that a write past it is seen)
  const size_t cap = 1u << 16;
  std::unique_ptr<uint64_t[]> out(new uint64_t[cap]); // (exactly the capacity handed over)
  for (uint32_t bits = 8; bits <= 15; bits++)
    for (uint32_t states : {32u, 64u})
    {
      for (uint32_t n_chains : kChains)
      {
        g_where = std::string(list_name) + " cus=" + std::to_string(dg.num_cus) + " lds=" + std::to_string(dg.max_lds) + " sets=" + std::to_string(dg.n_weight_sets) +
                  " bits=" + std::to_string(bits) + " states=" + std::to_string(states) + " chains=" + std::to_string(n_chains);
        PlanHeader h{};
        h.states = states, h.bits = bits, h.n_chains = h.n_pieces = n_chains, h.decoded_len = (uint64_t)n_chains * states * 32;
        // waves that build their own tables, and the same as an index pass; a block_ walk
        check_choice(tn, h, dg, LaunchFacts{}, "own tables");
        LaunchFacts pass;
        pass.index_pass = true;
        check_choice(tn, h, dg, pass, "index pass");
        PlanHeader walk = h;
        walk.flags = kPlanWalk;
        check_choice(tn, walk, dg, LaunchFacts{}, "walk");
        // raw plans with an index: one chain per wave, uniform intervals
        h.shared_hist = 1;
        for (uint32_t interval : {0u, 8u, 32u})
        {
          const TableChoice tc = choose_table(tn, bits, states, interval == 0);
          LaunchFacts f;
          f.persistent = true, f.table_mode = tc.mode, f.dual = tc.dual, f.interval = interval;
          PlanHeader hi = h;
          hi.interval = interval;
          check_choice(tn, hi, dg, f, interval == 0 ? "direct" : interval == 8 ? "persist 8" : "persist 32");
          f.calibrating = true;
          check_choice(tn, hi, dg, f, "calibrating");
          f.table_mode = 0; // (a plan without a host-built table)
          check_choice(tn, hi, dg, f, "no host table");
        }
        LaunchFacts single;
        single.single_valid = true, single.single_ring_entries = 2048;
        check_choice(tn, h, dg, single, "single");
        h.shared_hist = 0;
        // block_/mt_ plans with checkpoints: the block lists, dealt where the dealing takes them
        for (uint32_t n_blocks : block_counts)
        {
          if (n_blocks > n_chains)
            continue;
          std::vector<uint32_t> begin(n_blocks + 1);
          uint32_t fewest = n_chains;
          for (uint32_t k = 0; k <= n_blocks; k++)
            begin[k] = (uint32_t)((uint64_t)n_chains * k / n_blocks);
          for (uint32_t k = 0; k + 1 < n_blocks; k++)
            fewest = std::min(fewest, begin[k + 1] - begin[k]);
          for (uint32_t interval : {8u, 32u})
          {
            PlanHeader hg = h;
            hg.interval = interval, hg.decoded_len = (uint64_t)n_chains * states * interval;
            const std::string keep = g_where;
            g_where += " blocks=" + std::to_string(n_blocks) + " interval=" + std::to_string(interval);
            uint32_t weights[8];
            const bool dealt = deal_shares(tn, dg, begin.data(), n_blocks, n_chains, (uint64_t)n_chains * interval, bits, table.get(), weights);
            (dealt ? g_dealt : g_not_dealt)++;
            if (dealt)
            {
              CHECK(grid <= kDealtGridMax && table->begin[0] == 0 && table->begin[grid] == n_chains);
              for (uint32_t b = 0; b < grid; b++)
                CHECK(table->begin[b + 1] >= table->begin[b] && table->begin[b + 1] - table->begin[b] <= 0xFFFE);
            }
            for (uint32_t per_block : {1u, 8u})
              for (int lean = 0; lean < 2; lean++)
              {
                LaunchFacts f;
                f.n_groups = n_blocks * per_block, f.groups_lean = lean != 0, f.tickets = true, f.spread_min_block = lean ? fewest : 0;
                check_choice(tn, hg, dg, f, lean ? "grouped lean" : "grouped");
                if (!lean)
                  continue;
                f.dealt = dealt;
                memcpy(f.dealt_weights, weights, sizeof(weights));
                check_choice(tn, hg, dg, f, "grouped lean with its dealing");
                f.parts = true, f.n_parts = 4;
                check_choice(tn, hg, dg, f, "sub-runs");
              }
            g_shapes++;
            const BatchGroupShape bg = batch_grouped_shape(tn, dg, bits, n_blocks, n_blocks == 1 ? (uint64_t)n_chains << 13 : n_chains);
            CHECK(bg.grid >= 1 && bg.waves >= 1);
            g_where = keep;
          }
        }
        // the gather shapes: tasks as many as the plan has chains
        for (uint32_t table_mode : {0u, (uint32_t)kModePack64, (uint32_t)kModeRank, (uint32_t)kModeSpill})
        {
          const GatherShape g = gather_shape(tn, h, dg, table_mode, n_chains);
          const GatherShape gr = gather_ranges_shape(tn, h, dg, table_mode, n_chains, (uint64_t)n_chains * 4096, n_chains % 2 ? 4096 : 0);
          const GatherShape gs = gather_set_shape(dg, g.mode, g.shared, gather_table_bytes(g.mode, bits), n_chains);
          const GatherShape gsr = gather_set_ranges_shape(dg, g.mode, g.shared, gather_table_bytes(g.mode, bits), n_chains, (uint64_t)n_chains * 4096, n_chains % 2 ? 4096 : 0, 1 + n_chains % 7);
          g_shapes += 4;
          CHECK(g.waves >= 1 && gr.waves >= 1 && gs.waves >= 1 && gsr.waves >= 1 && gr.grid >= 1 && gsr.grid >= 1);
        }
      }
      // one chain per wave: the index of a stream that has the device to itself, and the batch launch's shape
      for (uint64_t total_groups : {(uint64_t)0, (uint64_t)1, (uint64_t)31, (uint64_t)32, (uint64_t)63 * 32, (uint64_t)46875, (uint64_t)1562500, (uint64_t)1 << 24})
      {
        g_where = std::string(list_name) + " cus=" + std::to_string(dg.num_cus) + " lds=" + std::to_string(dg.max_lds) + " sets=" + std::to_string(dg.n_weight_sets) +
                  " bits=" + std::to_string(bits) + " states=" + std::to_string(states) + " direct_boundaries of " + std::to_string(total_groups) + " groups";
        const size_t chains = direct_boundaries(tn, dg, states, bits, total_groups, out.get(), cap);
        g_indexes++;
        CHECK(chains >= 1 && chains - 1 <= cap); // (0: the capacity — there is room for every wave of these devices)
        for (size_t k = 0; k + 1 < chains; k++)
          CHECK(out[k] % 4 == 0 && out[k] < total_groups && (k == 0 ? out[k] > 0 : out[k] > out[k - 1]));
        const BatchShape bs = batch_direct_shape(tn, dg, bits, total_groups, states);
        g_shapes++;
        CHECK(bs.grid >= 1 && bs.waves >= 1);
      }
    }
}

int main()
{
  std::vector<DeviceGeom> devices;
  for (uint32_t cus : {1u, 8u, 80u, 255u, 256u, 304u})
    for (uint32_t lds : {64u * 1024, 160u * 1024})
    {
      DeviceGeom dg{};
      dg.num_cus = cus, dg.max_lds = lds;
      devices.push_back(dg);
    }
  DeviceGeom fitted = default_geom(); // an MI355X after hsrans_ctx_calibrate and hsrans_ctx_calibrate_runs
  fitted.have_direct_weights = 1, fitted.n_weight_sets = 2, fitted.set_run[0] = 96, fitted.set_run[1] = 400;
  for (uint32_t k = 0; k < 8; k++)
    fitted.direct_weights[k] = fitted.set_weights[0][k] = kNamed[1][k], fitted.set_weights[1][k] = 1000;
  devices.push_back(fitted);

  std::vector<std::pair<std::string, std::vector<uint32_t>>> lists;
  lists.push_back({"default", {}});
  const char *names[4] = {"flat", "steep", "reversed", "edge"};
  for (int k = 0; k < 4; k++)
    lists.push_back({names[k], std::vector<uint32_t>(kNamed[k], kNamed[k] + 8)});
  for (int k = 0; k < 32; k++)
  {
    std::vector<uint32_t> ws(8);
    std::string name = "random";
    for (uint32_t &w : ws)
      w = 100 + rnd(2901), name += " " + std::to_string(w);
    lists.push_back({name, ws});
  }
  for (const auto &list : lists)
  {
    const Tuning tn = tuning_under(list.second.empty() ? nullptr : list.second.data());
    if (!list.second.empty() && (!tn.dealt_weights_set || !tn.batch_weights_set || !tn.direct_weights_set))
    {
      printf("read_tuning did not take the list %s\n", list.first.c_str());
      return 1;
    }
    for (const DeviceGeom &dg : devices)
      sweep(tn, dg, list.first.c_str());
  }
  if (g_dealt < 100 || g_not_dealt < 100 || g_refused < 100)
  {
    printf("the sweep misses a kind of case: dealt %lu not dealt %lu refused %lu of %lu choices\n", g_dealt, g_not_dealt, g_refused, g_choices);
    return 1;
  }
  printf("%lu choices (%lu refused), %lu dealings (%lu dealt), %lu indexes, %lu shapes\n", g_choices, g_refused, g_dealt + g_not_dealt, g_dealt, g_indexes, g_shapes);
  printf("launch policy ok\n");
  return 0;
}
"""


def test_launch_policy_under_the_sanitizers(tmp_path):
    src = tmp_path / "launch_policy_check.cpp"
    exe = tmp_path / "launch_policy_check"
    src.write_text(PROGRAM)
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, str(src)]
    base += [os.path.join(CSRC, unit) for unit in UNITS] + ["-o", str(exe)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:  # a host compiler without the sanitizer runtimes: the same program, plain
        r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("launch policy ok"), (r.stdout[-2000:], r.stderr[-3000:])


MOVED = ("choose_table", "build_rank_table", "rank_table_entries", "pack64_max_bits", "launch_shape", "choose_launch", "launch_facts", "launch_info_of", "static_shares",
         "dealt_eligible", "dealt_lds", "deal_shares", "dealt_weights_now", "direct_weights_for", "direct_boundaries", "spread_longest_share_of", "class_cum_of",
         "cum_from_weights", "group_cum_of", "batch_direct_shape", "batch_grouped_shape", "gather_waves", "gather_shape", "gather_set_shape", "gather_ranges_shape",
         "gather_set_ranges_shape", "gather_table_bytes", "default_geom", "index_pass_mode", "index_fill_rows")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _definitions(text, name):
    """definitions of a function at namespace scope: its name at the start of a declarator on an unindented line that does not end in ';'"""
    return [line for line in text.splitlines() if re.match(r"^[A-Za-z_][\w:<> \*&]*\b%s\(" % name, line) and not line.rstrip().endswith(";")]


def test_the_policy_unit_names_no_kernel_and_the_kernel_file_no_policy():
    """What hsrans_launch.cpp took out of hsrans_kernels.hip stays out: the unit has no kernel, no launch, no HIP runtime call and no function
    that takes a stream, and includes no part of the device translation unit but kernels_layout.h; the kernel file defines none of the
    policy's functions."""
    launch, kernels = _read("hsrans_launch.cpp"), _read("hsrans_kernels.hip")
    code = re.sub(r"//[^\n]*", "", launch)  # (the comments may speak of kernels and launches)
    for word in ("hipLaunchKernelGGL", "__global__", "hipFuncSetAttribute", "hipStream_t", "<<<", "hipGetLastError", "hipMalloc", "hipMemcpy", "hipGetDevice"):
        assert word not in code, word
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code), "a HIP runtime call in hsrans_launch.cpp"
    includes = re.findall(r'#include\s+"(kernels_\w+\.h)"', launch)
    assert includes == ["kernels_layout.h"], includes
    for header in ("hsrans_launch.h", "kernels_layout.h"):
        text = re.sub(r"//[^\n]*", "", _read(header))
        assert "__global__" not in text and "hipStream_t" not in text and not re.findall(r'#include\s+"(kernels_\w+\.h)"', text), header
    assert "__device__ __forceinline__" not in _read("kernels_layout.h") and "__builtin_amdgcn" not in _read("kernels_layout.h")
    defined_here = [name for name in MOVED if _definitions(launch, name)]
    assert sorted(defined_here) == sorted(set(MOVED) - {"cum_from_weights", "group_cum_of"}), sorted(set(MOVED) - set(defined_here))
    for name in MOVED:
        assert not _definitions(kernels, name), name
    assert '#include "hsrans_launch.h"' in _read("hsrans_kernels.h")
