"""csrc/planes_cut.h on its own: the rules of one element range that the host's cut of hsrans_decode_device_planes_gather and the device's
(k_planes_cut, k_planes_merge_indirect) share.  A stand-alone program, compiled by the host compiler with nothing but that header (so the header
needs no HIP), walks the DEVICE's route over seeded random range lists: first_task[] and B_r by a sequential prefix of planes_range_tasks and
planes_range_slot, then for every task t below the total the last r with first_task[r] <= t by binary search and planes_task_at of it.  The test
compares what it prints, entry for entry, with hsrans_planes_gather_tasks of the same lists — the host's cut.  The range check is held against
the rows the host entry refuses (tests/test_gpu_planes_gather.py's `bad` list) and against hsrans_planes_gather_tasks' own refusals.

The program runs under AddressSanitizer and UBSan where the host compiler has them (it loads nothing into Python)."""
import os
import subprocess

import numpy as np
import pytest

import hypersonic_rans_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
ELEMENTS = 300_007  # not a multiple of 16
N_OUT = 5012        # the output's elements in the refusal rows

# (offset, length, dst_offset, accepted): the host entry's refusals, then rows it takes
CHECKS = [
    (ELEMENTS, 1, 0, False), (ELEMENTS - 4, 5, 0, False), (ELEMENTS + 1, 0, 0, False), (2**64 - 2, 4, 0, False),  # beyond the tensor; offset + length wraps
    (0, 16, N_OUT - 15, False), (0, 16, 2**64 - 8, False), (0, 16, 1 << 62, False), (0, 0, N_OUT + 1, False),     # beyond the output; dst_offset + length wraps
    (2**64 - 1, 2**64 - 1, 0, False), (0, 2**64 - 1, 0, False),
    (ELEMENTS, 0, 0, True), (0, 0, N_OUT, True), (ELEMENTS - 16, 16, N_OUT - 16, True), (0, N_OUT, 0, True), (7, 0, 3, True),
]

PROGRAM = r"""
#include "planes_cut.h"

#include <stdio.h>
#include <vector>

struct Task
{
  uint64_t src, work_pos;
  int64_t dst_delta;
  uint32_t lo, hi;
};
struct Range
{
  uint64_t offset, length, dst_offset;
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(uint64_t n) // [0, n)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (rng_state >> 11) % n;
}

static const uint64_t kElements = @ELEMENTS@, kOut = @N_OUT@;
static const uint64_t kLengths[] = {0, 1, 15, 16, 17, 4095, 4096, 4097};
static const uint64_t kPhases[] = {0, 1, 15};

// the device's route: k_planes_cut's prefix, then k_planes_merge_indirect's search and planes_task_at for every task
static int walk(const std::vector<Range> &list)
{
  const uint32_t n = (uint32_t)list.size();
  std::vector<uint32_t> first_task(n + 1);
  std::vector<uint64_t> base(n);
  uint64_t at = 0, tasks = 0;
  printf("L %u\n", n);
  for (uint32_t r = 0; r < n; r++)
  {
    const Range &g = list[r];
    if (!planes_source_ok(g.offset, g.length, kElements))
    {
      printf("the generator made a range beyond the tensor\n");
      return 1;
    }
    printf("R %llu %llu %llu\n", (unsigned long long)g.offset, (unsigned long long)g.length, (unsigned long long)g.dst_offset);
    first_task[r] = (uint32_t)tasks;
    base[r] = at;
    at += planes_range_slot(g.offset, g.length);
    tasks += planes_range_tasks(g.offset, g.length);
  }
  first_task[n] = (uint32_t)tasks;
  for (uint32_t t = 0; t < (uint32_t)tasks; t++)
  {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1)
    {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (first_task[mid] <= t)
        lo = mid;
      else
        hi = mid;
    }
    const Range &g = list[lo];
    const Task k = planes_task_at<Task>(g.offset, g.length, g.dst_offset, base[lo], t - first_task[lo]);
    printf("T %llu %llu %llu %u %u\n", (unsigned long long)k.src, (unsigned long long)k.work_pos, (unsigned long long)k.dst_delta, k.lo, k.hi);
  }
  printf("S %llu\n", (unsigned long long)at);
  return 0;
}

int main()
{
  // every phase with every length, one range per list and all of them in one list
  std::vector<Range> all;
  for (uint64_t phase : kPhases)
    for (uint64_t len : kLengths)
    {
      const Range g{16 * (1 + rnd(1000)) + phase, len, rnd(1 << 20)};
      all.push_back(g);
      if (walk({g}))
        return 1;
    }
  if (walk(all))
    return 1;
  // ranges that end at the tensor's last element, alone and behind others
  for (uint64_t len : kLengths)
    if (walk({Range{kElements - len, len, 3}}) || walk({Range{5, 0, 0}, Range{31, 4097, 100}, Range{kElements - len, len, 1 << 30}}))
      return 1;
  if (walk({}))
    return 1;
  // seeded random lists: short and long ranges, empty ones between them, destinations below and above the source
  for (int c = 0; c < 60; c++)
  {
    std::vector<Range> list(1 + rnd(40));
    for (Range &g : list)
    {
      const uint64_t len = rnd(4) == 0 ? kLengths[rnd(8)] : rnd(8) == 0 ? rnd(40000) : rnd(600);
      g.length = len > kElements ? kElements : len;
      g.offset = rnd(5) == 0 ? kElements - g.length : rnd(kElements - g.length + 1);
      g.dst_offset = rnd(1 << 22);
    }
    if (walk(list))
      return 1;
  }
  // the range check
  static const struct
  {
    uint64_t offset, length, dst_offset;
  } checks[] = {@CHECKS@};
  for (const auto &c : checks)
    printf("C %d\n", (int)(planes_source_ok(c.offset, c.length, kElements) && planes_dest_ok(c.dst_offset, c.length, kOut)));
  printf("cut ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("planes_cut")
    src, exe = tmp / "planes_cut_check.cpp", tmp / "planes_cut_check"
    checks = ", ".join("{%dull, %dull, %dull}" % (o, n, d) for o, n, d, _ in CHECKS)
    src.write_text(PROGRAM.replace("@ELEMENTS@", str(ELEMENTS)).replace("@N_OUT@", str(N_OUT)).replace("@CHECKS@", checks))
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:  # a host compiler without the sanitizer runtimes: the same program, plain
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("cut ok"), (r.stdout[-2000:], r.stderr[-3000:])
    lists, checks_out = [], []
    for line in r.stdout.splitlines():
        kind, *rest = line.split()
        if kind == "L":
            lists.append({"ranges": [], "tasks": [], "slots": None})
        elif kind == "R":
            lists[-1]["ranges"].append(tuple(int(v) for v in rest))
        elif kind == "T":
            lists[-1]["tasks"].append(tuple(int(v) for v in rest))
        elif kind == "S":
            lists[-1]["slots"] = int(rest[0])
        elif kind == "C":
            checks_out.append(bool(int(rest[0])))
    return lists, checks_out


def test_the_devices_route_gives_the_hosts_cut(printed):
    lists, _ = printed
    assert len(lists) > 100
    for case in lists:
        want = H.planes_gather_tasks(case["ranges"], ELEMENTS)
        assert [tuple(int(v) for v in row) for row in want] == case["tasks"], case["ranges"]
        assert case["slots"] == sum((off % 16 + n + 15) // 16 * 16 if n else 0 for off, n, _ in case["ranges"])
        assert case["slots"] <= sum(n for _, n, _ in case["ranges"]) + 30 * len(case["ranges"])


def test_the_lists_hit_every_phase_length_and_the_tensors_end(printed):
    lists, _ = printed
    ranges = [g for case in lists for g in case["ranges"]]
    for phase in (0, 1, 15):
        for n in (0, 1, 15, 16, 17, 4095, 4096, 4097):
            assert any(off % 16 == phase and length == n for off, length, _ in ranges), (phase, n)
    assert any(off + n == ELEMENTS and n > 0 for off, n, _ in ranges)
    assert any(len(case["tasks"]) > 8 and len(case["ranges"]) > 8 for case in lists)  # the search has something to search
    assert any(n == 0 for _, n, _ in ranges) and any(len(case["ranges"]) == 0 for case in lists)


def test_the_range_check_is_the_host_entrys(printed):
    _, got = printed
    assert got == [ok for *_, ok in CHECKS]
    # ... and where the source alone decides, hsrans_planes_gather_tasks (the host entry's own check) says the same
    L = H.load_library()
    for off, n, dst, ok in CHECKS:
        arr = np.asarray([(off, n, dst)], np.uint64)
        source_ok = off <= ELEMENTS and n <= ELEMENTS - off
        assert (not ok) or source_ok
        tasks = L.hsrans_planes_gather_tasks(arr.ctypes.data, 1, ELEMENTS, None, 0)
        assert tasks == ((off % 16 + n + 4095) // 4096 if source_ok and n else 0), (off, n)
