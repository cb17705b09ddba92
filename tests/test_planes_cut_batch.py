"""csrc/planes_cut_batch.h on its own: the rules of one row of hsrans_decode_device_planes_gather_batch that the host's cut (measure_rows) and the
device's (k_planes_cut_batch, k_planes_merge_batch_indirect) share.  A stand-alone program, compiled by the host compiler with nothing but that
header and planes_cut.h (so neither needs HIP), walks the DEVICE's route over row lists of members of mixed element sizes: C_r, first_task[] and
the gather rows by a sequential prefix of planes_row_cut through planes_rows_add, then for every task t below the total the last r with
first_task[r] <= t by binary search and planes_task_at of it with base C_r and plane_step = slot_r.  The test compares what it prints, entry
for entry, with hsrans_planes_gather_batch_tasks of the same lists — the host's cut — and the verdict on every list with a model in Python's
unbounded integers.  Two refusals that cannot be provoked cheaply on a GPU are covered here: an offset + length that wraps 2^64 and a task
total that crosses 2^31 (hsrans_planes_gather_batch_tasks counts without walking, so the lists just below the limit are compared by count).

The program runs under AddressSanitizer and UBSan where the host compiler has them (it loads nothing into Python)."""
import os
import subprocess

import numpy as np
import pytest

import hypersonic_rans_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
# (element size, elements, coded planes) per member; the last two are far larger than any memory: only counted, never walked
MEMBERS = [(2, 300_007, 2), (4, 70_001, 3), (8, 20_003, 5), (2, 4_099, 0), (4, 16, 4), (2, 1 << 45, 1), (8, (1 << 64) - 1, 8)]
HUGE, WHOLE = 5, 6
LIMIT = 1 << 31
OUT_CAPACITY = 40_096  # bytes, in the destination checks

# (member, dst_offset, length, accepted): (dst_offset + length) * W against OUT_CAPACITY
DEST_CHECKS = [
    (0, 20_048, 0, True), (0, 20_047, 1, True), (0, 20_048, 1, False), (1, 10_024, 0, True), (1, 10_009, 16, False), (2, 5_012, 0, True), (2, 5_011, 1, True),
    (2, 4_997, 16, False), (0, 2**64 - 8, 16, False), (2, 1 << 62, 16, False), (1, 1 << 62, 0, False), (0, 0, 20_048, True), (2, 0, 5_013, False),
]

PROGRAM = r"""
#include "planes_cut_batch.h"

#include <stdio.h>
#include <vector>

struct Task
{
  uint64_t src, work_pos;
  int64_t dst_delta;
  uint32_t lo, hi;
};
struct Row
{
  uint64_t offset, length, dst_offset;
  uint32_t member, reserved;
};
struct Member
{
  uint32_t W;
  uint64_t elements;
  uint32_t coded;
};
static const Member kMembers[] = {@MEMBERS@};
static const uint32_t kCount = sizeof(kMembers) / sizeof(kMembers[0]), kHuge = @HUGE@, kWhole = @WHOLE@;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(uint64_t n) // [0, n)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (rng_state >> 11) % n;
}

static const uint64_t kLengths[] = {0, 1, 15, 16, 17, 4095, 4096, 4097};

// the device's route: k_planes_cut_batch's prefix, then k_planes_merge_batch_indirect's search and planes_task_at for every task
static void walk(const std::vector<Row> &list)
{
  const uint32_t n = (uint32_t)list.size();
  std::vector<uint32_t> first_task(n + 1);
  std::vector<uint64_t> base(n);
  PlanesRowsSum sum{0, 0, 0};
  bool ok = true;
  printf("L %u\n", n);
  for (uint32_t r = 0; r < n; r++)
  {
    const Row &g = list[r];
    printf("R %u %llu %llu %llu %u\n", g.member, (unsigned long long)g.offset, (unsigned long long)g.length, (unsigned long long)g.dst_offset, g.reserved);
    if (!ok)
      continue;
    PlanesRowCut cut;
    first_task[r] = (uint32_t)sum.tasks;
    base[r] = sum.work;
    ok = g.member < kCount && g.reserved == 0 && planes_row_cut(g.offset, g.length, kMembers[g.member].elements, kMembers[g.member].W, kMembers[g.member].coded, &cut) &&
         planes_rows_add(&sum, cut);
  }
  if (!ok)
  {
    printf("V 0 0 0 0\n");
    return;
  }
  first_task[n] = (uint32_t)sum.tasks;
  printf("V 1 %llu %llu %llu\n", (unsigned long long)sum.tasks, (unsigned long long)sum.work, (unsigned long long)sum.rows);
  if (sum.tasks > 100000) // (only counted)
    return;
  for (uint32_t t = 0; t < (uint32_t)sum.tasks; t++)
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
    const Row &g = list[lo];
    const Task k = planes_task_at<Task>(g.offset, g.length, g.dst_offset, base[lo], t - first_task[lo]);
    printf("T %llu %llu %llu %llu %u %u %u\n", (unsigned long long)k.src, (unsigned long long)k.work_pos, (unsigned long long)planes_range_slot(g.offset, g.length),
           (unsigned long long)k.dst_delta, k.lo, k.hi, g.member);
  }
}

static Row row_of(uint32_t m, uint64_t len, uint64_t phase)
{
  const uint64_t elements = kMembers[m].elements;
  if (len > elements)
    len = elements;
  uint64_t offset = rnd(5) == 0 ? elements - len : rnd(elements - len + 1);
  if (phase < 16 && (elements - len) / 16 != 0) // (16 (room - 1) + 15 + len <= elements)
    offset = 16 * rnd((elements - len) / 16) + phase;
  return Row{offset, len, rnd(1 << 22), m, 0};
}

int main()
{
  const uint32_t kSmall = 5; // members 0 .. 4 can be walked
  // every phase with every length over the element sizes, one row per list and all of them in one list
  std::vector<Row> all;
  for (uint64_t phase = 0; phase < 16; phase++)
    for (uint64_t len : kLengths)
    {
      const Row g = row_of((uint32_t)((phase + len) % 3), len, phase);
      all.push_back(g);
      walk({g});
    }
  walk(all);
  walk({});
  // rows that end with their member, alone and behind others of other element sizes
  for (uint32_t m = 0; m < kSmall; m++)
    for (uint64_t len : kLengths)
    {
      const uint64_t n = len > kMembers[m].elements ? kMembers[m].elements : len;
      walk({Row{kMembers[m].elements - n, n, 3, m, 0}});
      walk({Row{5, 0, 0, 2, 0}, Row{31, 4097, 100, 0, 0}, Row{kMembers[m].elements - n, n, 1 << 30, m, 0}, Row{0, 16, 7, 4, 0}});
    }
  // seeded random lists: short and long rows over all members, empty ones between them
  for (int c = 0; c < 80; c++)
  {
    std::vector<Row> list(1 + rnd(40));
    for (Row &g : list)
      g = row_of((uint32_t)rnd(kSmall), rnd(4) == 0 ? kLengths[rnd(8)] : rnd(8) == 0 ? rnd(40000) : rnd(600), rnd(3) == 0 ? rnd(16) : 16);
    walk(list);
  }
  // what a row is refused for, first, last and between good rows; the good rows alone pass
  const Row good0{100, 5000, 0, 0, 0}, good1{7, 0, 3, 2, 0}, good2{20003 - 9, 9, 1300, 2, 0};
  const Row refused[] = {
      {0, 1, 0, kCount, 0},                         // member = members
      {0, 0, 0, kCount, 0},                         // ... of an empty row too
      {0, 1, 0, 0xFFFFFFFFu, 0},
      {0, 1, 0, 0, 1},                              // reserved
      {0, 0, 0, 0, 1},
      {300007 - 4, 5, 0, 0, 0},                     // beyond its member
      {70001, 1, 0, 1, 0},
      {20004, 0, 0, 2, 0},                          // an empty row one beyond the end
      {0xFFFFFFFFFFFFFFFEull, 4, 0, 0, 0},          // offset + length wraps 2^64
      {0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull, 0, kWhole, 0},
      {0xFFFFFFFFFFFFFFF0ull, 32, 0, kWhole, 0},
      {15, 0xFFFFFFFFFFFFFFF0ull, 0, kWhole, 0},    // inside the member; phase + length cannot be rounded up to 16
      {0, 0x2000000000000000ull, 0, kWhole, 0},     // W * slot wraps
  };
  walk({good0, good1, good2});
  for (const Row &bad : refused)
  {
    walk({bad});
    walk({bad, good0, good1, good2});
    walk({good0, good1, bad, good2});
    walk({good0, good1, good2, bad});
  }
  walk({Row{70001, 0, 0, 1, 0}, Row{20003, 0, 9, 2, 0}}); // empty rows AT their members' ends pass
  // sums: W * slot wraps over two rows that pass alone; a task total crossing 2^31
  const Row quarter{0, 0x0800000000000000ull, 0, kWhole, 0}; // 8 * 2^59 = 2^62 bytes, 2^47 tasks: refused by the task total alone
  walk({quarter});
  const uint64_t kTask = 4096;
  const Row big{16, (1ull << 30) * kTask, 0, kHuge, 0};           // exactly 2^30 tasks
  const Row most{0, ((1ull << 30) - 1) * kTask, 0, kHuge, 0};     // 2^30 - 1
  const Row one{16 * 9 + 3, 4090, 5, 0, 0};                        // 1 task
  walk({big});
  walk({big, most});            // 2^31 - 1: the most a call can have
  walk({big, most, one});       // 2^31
  walk({big, one, big});        // 2^31 + 1
  walk({one, big, good1, most}); // 2^31 again, the crossing row last
  walk({big, big});
  walk({Row{1, (1ull << 31) * kTask - 1, 0, kHuge, 0}});           // phase 1: 2^31 tasks in one row
  walk({Row{0, (1ull << 31) * kTask - kTask, 0, kHuge, 0}});       // 2^31 - 1 in one row
  // the gather rows' limit, on the sums themselves (2^31 / 8 rows cannot be walked here)
  {
    PlanesRowsSum sum{0, 0, (1ull << 31) - 9};
    const PlanesRowCut eight{16, 128, 1, 8};
    const bool first = planes_rows_add(&sum, eight), second = planes_rows_add(&sum, eight);
    PlanesRowsSum wrap{0xFFFFFFFFFFFFFF00ull, 0, 0};
    const PlanesRowCut a{64, 128, 1, 2}, b{128, 256, 1, 2};
    const bool third = planes_rows_add(&wrap, a), fourth = planes_rows_add(&wrap, b);
    printf("A %d %d %d %d %llu\n", (int)first, (int)second, (int)third, (int)fourth, (unsigned long long)sum.rows);
  }
  // the destination rule
  static const struct
  {
    uint32_t member;
    uint64_t dst_offset, length;
  } checks[] = {@DEST_CHECKS@};
  for (const auto &c : checks)
    printf("C %d\n", (int)planes_row_dest_ok(c.dst_offset, c.length, kMembers[c.member].W, @OUT_CAPACITY@));
  printf("D %d %d %d\n", (int)planes_row_dest_ok(0, 0, 3, 64), (int)planes_row_dest_ok(0, 0, 0, 64), (int)planes_width_ok(16));
  printf("cut ok\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("planes_cut_batch")
    src, exe = tmp / "planes_cut_batch_check.cpp", tmp / "planes_cut_batch_check"
    members = ", ".join("{%du, %dull, %du}" % m for m in MEMBERS)
    checks = ", ".join("{%du, %dull, %dull}" % (m, d, n) for m, d, n, _ in DEST_CHECKS)
    text = PROGRAM.replace("@MEMBERS@", members).replace("@HUGE@", str(HUGE)).replace("@WHOLE@", str(WHOLE)).replace("@DEST_CHECKS@", checks)
    src.write_text(text.replace("@OUT_CAPACITY@", str(OUT_CAPACITY)))
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:  # a host compiler without the sanitizer runtimes: the same program, plain
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("cut ok"), (r.stdout[-2000:], r.stderr[-3000:])
    lists, dest, sums, widths = [], [], None, None
    for line in r.stdout.splitlines():
        kind, *rest = line.split()
        if kind == "L":
            lists.append({"rows": [], "tasks": [], "verdict": None})
        elif kind == "R":
            lists[-1]["rows"].append(tuple(int(v) for v in rest))
        elif kind == "T":
            lists[-1]["tasks"].append(tuple(int(v) for v in rest))
        elif kind == "V":
            lists[-1]["verdict"] = tuple(int(v) for v in rest)
        elif kind == "C":
            dest.append(bool(int(rest[0])))
        elif kind == "A":
            sums = [int(v) for v in rest]
        elif kind == "D":
            widths = [int(v) for v in rest]
    return lists, dest, sums, widths


def _model(rows):
    """the header's contract in unbounded integers: None where the call is refused, else (tasks, sum of W * slot, gather rows)"""
    tasks = work = grows = 0
    for m, off, n, _, reserved in rows:
        if m >= len(MEMBERS) or reserved != 0:
            return None
        W, elements, coded = MEMBERS[m]
        if off + n > elements or off % 16 + n > 2**64 - 16:
            return None
        slot = (off % 16 + n + 15) // 16 * 16 if n else 0
        work += W * slot
        tasks += (off % 16 + n + 4095) // 4096 if n else 0
        grows += coded if n else 0
        if work >= 2**64 or tasks >= LIMIT or grows >= LIMIT:
            return None
    return tasks, work, grows


def _host_count(rows):
    arr = np.zeros(len(rows), np.dtype([("offset", "<u8"), ("length", "<u8"), ("dst_offset", "<u8"), ("member", "<u4"), ("reserved", "<u4")]))
    for k, (m, off, n, dst, reserved) in enumerate(rows):
        arr[k] = (off, n, dst, m, reserved)
    sizes, elems = np.asarray([m[0] for m in MEMBERS], np.uint32), np.asarray([m[1] for m in MEMBERS], np.uint64)
    return H.load_library().hsrans_planes_gather_batch_tasks(arr.ctypes.data if len(rows) else None, len(rows), sizes.ctypes.data, elems.ctypes.data, len(MEMBERS), None, 0)


def test_the_devices_route_gives_the_hosts_cut(printed):
    lists = printed[0]
    assert len(lists) > 300
    walked = 0
    for case in lists:
        want = _model(case["rows"])
        assert case["verdict"] == ((1,) + want if want is not None else (0, 0, 0, 0)), case["rows"]
        assert _host_count(case["rows"]) == (want[0] if want is not None else 0), case["rows"]  # the host's cut refuses, and counts, alike
        if want is None or want[0] > 100_000:
            assert case["tasks"] == []
            continue
        host = H.planes_gather_batch_tasks([(m, off, n, dst) for m, off, n, dst, _ in case["rows"]], [m[0] for m in MEMBERS], [m[1] for m in MEMBERS])
        assert [tuple(int(v) for v in row) for row in host] == case["tasks"], case["rows"]  # src, work_pos, plane_step, dst_delta, lo, hi, member
        assert want[1] <= sum(MEMBERS[m][0] * (n + 30) for m, _, n, _, _ in case["rows"])  # what hsrans_planes_gather_batch_workspace_bytes bounds
        walked += len(case["tasks"])
    assert walked > 2000


def test_the_lists_hit_every_phase_length_element_size_and_limit(printed):
    lists = printed[0]
    rows = [g for case in lists for g in case["rows"]]
    for phase in range(16):
        for n in (0, 1, 15, 16, 17, 4095, 4096, 4097):
            assert any(off % 16 == phase and length == n and m < 3 for m, off, length, _, _ in rows), (phase, n)
    for m in range(5):
        assert any(k == m and off + n == MEMBERS[m][1] and n > 0 for k, off, n, _, _ in rows), m
    assert any(len(case["tasks"]) > 8 and len({g[0] for g in case["rows"]}) >= 3 for case in lists)  # the search has rows of mixed sizes to search
    assert any(n == 0 for _, _, n, _, _ in rows) and any(len(case["rows"]) == 0 for case in lists)
    assert any(off + n >= 2**64 for _, off, n, _, _ in rows), "offset + length wraps 2^64"
    totals = {case["verdict"][1] for case in lists if case["verdict"][0]}
    assert LIMIT - 1 in totals and max(totals) == LIMIT - 1, "the most tasks a call can have pass"
    crossing = [case for case in lists if case["verdict"][0] == 0 and all(_model([g]) is not None for g in case["rows"])]
    assert len(crossing) >= 4, "lists whose rows pass alone and whose task total reaches 2^31"
    assert any(sum(_model([g])[0] for g in case["rows"]) == LIMIT for case in crossing)


def test_the_sums_refuse_at_their_limits(printed):
    _, _, sums, widths = printed
    # 2^31 - 9 + 8 gather rows pass, 8 more reach 2^31; a sum of W * slot that ends at 2^64 - 128 passes, one that wraps does not
    assert sums == [1, 0, 1, 0, (1 << 31) + 7]
    assert widths == [0, 0, 0]


def test_the_destination_rule_is_the_host_entrys(printed):
    assert printed[1] == [ok for *_, ok in DEST_CHECKS]
    for m, dst, n, ok in DEST_CHECKS:
        assert ok == ((dst + n) * MEMBERS[m][0] <= OUT_CAPACITY), (m, dst, n)
