// hsrans_planes_gather_batch_indirect.hip — hsrans_decode_device_planes_gather_batch_indirect: rows of MANY frames, in device memory, read
// when the launches run.  k_planes_cut_batch checks the rows against their members, lays out the workspace (C_r, the prefix of W * slot),
// counts the merge's tasks and writes, for every non-empty row, one row of the set's gather per coded plane of its member; behind the set's
// own indirect call k_planes_merge_batch_indirect interleaves the rows: it finds each task's row in the prefix the cut left, derives the task
// by planes_task_at (planes_cut.h) with base C_r and the sub-slot distance slot_r, and reads the member's record as the list-driven batch
// merge does (hsrans_planes_gather_batch.hip).  The row rules are planes_cut_batch.h's, which the host's cut uses too.  Control workspace:
// PlanesCutBatchWs (hsrans_planes.h).
// The merge's body is k_planes_merge_ranges_batch's, restated here (planes_shuffle.h says why).
#include "hsrans_planes.h"
#include "hsrans_plan.h"
#include "planes_cut_batch.h"
#include "planes_shuffle.h"

#include <algorithm>

namespace hsrans
{
namespace
{
using namespace planes_detail;

static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements && kPlanesCutTask == kPlanesGatherTaskElements, "one lane per 16-element block of a task");
static_assert(sizeof(PlanesSetRow) == 32 && sizeof(PlanesCutBatchMember) == 16 && sizeof(PlanesGatherBatchMember) == 72, "the rows' and the records' layout");

// ---------------------------------------------------------------------------------------------------------------
// One workgroup of 1024 threads, shaped like k_planes_cut: a round is kPlanesCutBatchRows consecutive rows per thread.  A row costs two
// dependent loads — the row, then its member's 16-byte cut record — so a round issues all its row loads together and then all its record
// loads together: the chain is paid once per 2048 rows.  W * slot (64-bit), the task counts and the gather rows are scanned inside the wave
// by __shfl_up, over the 16 waves through LDS, with carries from round to round; every total a thread needs is in its registers, so no word
// written here is read back here.  One row that fails planes_cut_batch.h's rules, a count above max_count, a sum of W * slot above the
// workspace or 2^31 tasks or gather rows refuse the whole call: the task total and the set's row count are written as 0 after the last round
// and kStatusBadRange is set.  Every word the set's launches and the merge read is written by every call.
// A refused row counts as empty, so whatever the rows hold the gather rows written stay inside rows[max_count * max_elem_size].
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPlanesCutBatchRows = 2;

__global__ void __launch_bounds__(1024) k_planes_cut_batch(PlanesCutBatchParams cp)
{
  __shared__ uint64_t wave_work[16], wave_tasks[16];
  __shared__ uint32_t wave_rows[16];
  __shared__ uint32_t any_bad;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t n = cp.count != nullptr ? *cp.count : cp.max_count;
  bool bad = n > cp.max_count;
  if (bad)
    n = 0;
  if (threadIdx.x == 0)
    any_bad = 0;
  __syncthreads();
  uint64_t work_carry = 0, task_carry = 0; // of the rounds before this one (the same on every thread)
  uint32_t row_carry = 0;                  // (at most max_count * max_elem_size < 2^31)
  for (uint64_t r0 = 0; r0 < n; r0 += 1024 * kPlanesCutBatchRows)
  {
    const uint64_t mine = r0 + (uint64_t)threadIdx.x * kPlanesCutBatchRows;
    PlanesSetRow g[kPlanesCutBatchRows];
    PlanesCutBatchMember m[kPlanesCutBatchRows];
    PlanesRowCut c[kPlanesCutBatchRows];
    uint64_t my_work = 0, my_tasks = 0;
    uint32_t my_rows = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatchRows; j++) // (no branch between the loads: rows beyond n read row 0 and do not count)
      g[j] = cp.ranges[mine + j < n ? mine + j : 0];
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatchRows; j++) // (... and a member beyond the set's reads record 0)
      m[j] = cp.members[g[j].member < cp.n_members ? g[j].member : 0];
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatchRows; j++)
    {
      const bool in = mine + j < n;
      const bool good = g[j].member < cp.n_members && g[j].reserved == 0 &&
                        planes_row_cut(g[j].offset, g[j].length, m[j].elements, m[j].W, (uint32_t)__builtin_popcount(m[j].coded_mask), &c[j]) &&
                        planes_row_dest_ok(g[j].dst_offset, g[j].length, m[j].W, cp.out_capacity) &&
                        c[j].work <= cp.work_limit; // (so that no sum below can wrap: work_limit <= 2^48)
      if (!in || !good)
        c[j] = PlanesRowCut{0, 0, 0, 0};
      bad = bad || (in && !good);
      my_work += c[j].work;
      my_tasks += c[j].tasks;
      my_rows += c[j].rows;
    }
    // inclusive scans of the threads' sums: inside the wave, then over the 16 waves' sums
    uint64_t incl_work = my_work, incl_tasks = my_tasks;
    uint32_t incl_rows = my_rows;
    for (uint32_t d = 1; d < 64; d *= 2)
    {
      const uint64_t w = __shfl_up(incl_work, d, 64), t = __shfl_up(incl_tasks, d, 64);
      const uint32_t q = __shfl_up(incl_rows, d, 64);
      if (lane >= d)
      {
        incl_work += w;
        incl_tasks += t;
        incl_rows += q;
      }
    }
    __syncthreads(); // (the sums of the round before have been read)
    if (lane == 63)
    {
      wave_work[wave] = incl_work;
      wave_tasks[wave] = incl_tasks;
      wave_rows[wave] = incl_rows;
    }
    __syncthreads();
    uint64_t at = work_carry, first = task_carry, round_work = 0, round_tasks = 0;
    uint32_t row_at = row_carry, round_rows = 0;
#pragma unroll 4 // (all 16 waves' sums read at once are 80 registers: the kernel would spill)
    for (uint32_t w = 0; w < 16; w++)
    {
      const uint64_t s = wave_work[w], t = wave_tasks[w];
      const uint32_t q = wave_rows[w];
      at += w < wave ? s : 0;
      first += w < wave ? t : 0;
      row_at += w < wave ? q : 0;
      round_work += s;
      round_tasks += t;
      round_rows += q;
    }
    at += incl_work - my_work;      // C_r of this thread's first row ...
    first += incl_tasks - my_tasks; // ... its first task (a prefix at or above the limits is refused below: what is stored then is never read) ...
    row_at += incl_rows - my_rows;  // ... and its first gather row
#pragma unroll
    for (uint32_t j = 0; j < kPlanesCutBatchRows; j++)
    {
      const uint64_t r = mine + j;
      if (r < n)
      {
        cp.first_task[r] = (uint32_t)first;
        cp.base[r] = at;
        cp.first_row[r] = row_at;
        if (c[j].rows != 0)
        {
          const uint64_t to = at + (g[j].offset & 15);
          uint32_t k = row_at, member = m[j].coded_at;
#pragma unroll 1
          for (uint32_t p = 0, mask = m[j].coded_mask; mask != 0; p++, mask >>= 1) // (a short loop kept rolled, as k_planes_cut's)
            if ((mask & 1) != 0)
              cp.rows[k++] = PlanesSetRow{g[j].offset, g[j].length, to + p * c[j].slot, member++, 0};
        }
      }
      at += c[j].work;
      first += c[j].tasks;
      row_at += c[j].rows;
    }
    work_carry += round_work;
    task_carry += round_tasks;
    row_carry += round_rows;
    if (work_carry > cp.work_limit)
    {
      bad = true;
      work_carry = 0;
    }
    if (task_carry >= kPlanesCutLimit)
    {
      bad = true;
      task_carry = 0;
    }
  }
  if (bad || row_carry >= kPlanesCutLimit)
    any_bad = 1; // (benign race: every writer stores 1)
  __syncthreads();
  if (threadIdx.x == 0)
  {
    const bool refuse = uni(any_bad) != 0; // (a scalar: it selects between scalars)
    cp.first_task[n] = (uint32_t)task_carry;
    cp.header[kPlanesWsTotal] = refuse ? 0 : (uint32_t)task_carry;
    cp.header[kPlanesWsCount] = n;
    cp.header[kPlanesWsRows] = refuse ? 0 : row_carry;
    if (refuse)
      atomicOr(cp.status, kStatusBadRange);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The merge.  Any grid: workgroup b serves tasks b, b + grid, ... below the total the cut left; a workgroup whose first task lies beyond it
// returns.  A task's row is the last r with first_task[r] <= t (rows without tasks share their successor's entry and are passed over),
// found by task_row (planes_shuffle.h).  The row, C_r and then the member's record are read the same on every lane, on scalar paths; the
// task is planes_task_at's with base C_r, its planes slot_r apart.  One branch on W into the body.
// ---------------------------------------------------------------------------------------------------------------

// the task as the workgroup holds it: every field the same on every lane
struct Task
{
  uint64_t src, work_pos, plane_step, dst_delta;
  uint32_t lo, hi;
};

// k_planes_merge_ranges<W>'s body for one task of a member of W-byte elements (k_planes_merge_ranges_batch's merge_task)
template <uint32_t W>
__device__ __forceinline__ void merge_task(const Task &t, const PlanesGatherBatchMember *m, const uint8_t *work, uint8_t *__restrict__ out)
{
  const uint32_t first = threadIdx.x * kLaneElements; // the lane's block: elements [src + first, src + first + 16)
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements; // (t.lo < 16: only lane 0 has a head)
  const uint32_t coded_mask = uni(m->coded_mask);
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
  {
    const uint64_t stored = uni64((uint64_t)m->stored[p]); // (read whether used or not: W loads at once, not one behind each branch)
    const uint64_t at = ((coded_mask >> p) & 1) != 0 ? (uint64_t)work + t.work_pos + p * t.plane_step : stored + t.src;
    src[p] = global_at(at) + first;
  }
  const uint64_t base = t.src + first + t.dst_delta; // the output element of the block's element 0 (modulo 2^64: a head's may lie below 0)
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
    merge16<W>(pl, e);
    uint8_t *dst = out + base * W;
    if (((uintptr_t)dst & 15) == 0)
    {
#pragma unroll
      for (uint32_t k = 0; k < W; k++)
        store16(dst + 16 * k, e + 4 * k);
    }
    else
      store_elements<W>(dst, e);
    return;
  }
  for (uint32_t i = lo; i < hi; i++)
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      out[(base + i) * W + p] = src[p][i];
}

__global__ __launch_bounds__(kThreads) void k_planes_merge_batch_indirect(const PlanesSetRow *__restrict__ ranges, const uint32_t *__restrict__ header,
                                                                          const uint32_t *__restrict__ first_task, const uint64_t *__restrict__ bases,
                                                                          const PlanesGatherBatchMember *__restrict__ members, const uint8_t *work, uint8_t *__restrict__ out)
{
  const uint32_t total = uni(header[kPlanesWsTotal]);
  if (blockIdx.x >= total)
    return;
  const uint32_t n = uni(header[kPlanesWsCount]);
  for (uint32_t t = blockIdx.x; t < total; t += gridDim.x)
  {
    const uint32_t r = task_row(first_task, n, t);
    const PlanesSetRow *row = ranges + r;
    const uint64_t offset = uni64(row->offset), length = uni64(row->length), dst_offset = uni64(row->dst_offset);
    const PlanesGatherBatchMember *m = members + uni(row->member);
    const PlanesGatherTask cut = planes_task_at<PlanesGatherTask>(offset, length, dst_offset, uni64(bases[r]), t - uni(first_task[r]));
    const Task task{cut.src, cut.work_pos, planes_range_slot(offset, length), (uint64_t)cut.dst_delta, cut.lo, cut.hi};
    const uint32_t W = uni(m->W);
    if (W == 2)
      merge_task<2>(task, m, work, out);
    else if (W == 4)
      merge_task<4>(task, m, work, out);
    else if (W == 8)
      merge_task<8>(task, m, work, out);
  }
}
} // namespace

// A workgroup is 4 waves, one per SIMD, so a CU holds as many workgroups as a SIMD holds waves of the kernel, which serves every element
// size and so has the registers of the 8-byte body (tests/test_planes_gather_batch_indirect_resources.py holds the compiler's report
// against this).
constexpr uint32_t kMergeBatchIndirectWavesPerSimd = 8;

uint32_t planes_merge_batch_indirect_grid(uint32_t num_cus, uint32_t min_W, uint32_t max_count, uint64_t work_bytes)
{
  const uint64_t most = (uint64_t)max_count + work_bytes / ((uint64_t)std::max(1u, min_W) * kPlanesGatherTaskElements);
  const uint64_t resident = (uint64_t)std::max(1u, num_cus) * kMergeBatchIndirectWavesPerSimd;
  return (uint32_t)std::max<uint64_t>(1, std::min(most, resident));
}

hipError_t launch_planes_cut_batch(const PlanesCutBatchParams &cp, hipStream_t stream)
{
  if (cp.ranges == nullptr || ((uintptr_t)cp.ranges & 7) != 0 || cp.members == nullptr || ((uintptr_t)cp.members & 15) != 0 || cp.max_count == 0 || cp.n_members == 0 ||
      cp.work_limit > ((uint64_t)1 << 48) || cp.header == nullptr || cp.first_task == nullptr || cp.first_row == nullptr || cp.base == nullptr || cp.rows == nullptr ||
      cp.status == nullptr)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_planes_cut_batch, dim3(1), dim3(1024), 0, stream, cp);
  return hipGetLastError();
}

hipError_t launch_planes_merge_batch_indirect(const PlanesSetRow *d_ranges, const uint32_t *d_header, const uint32_t *d_first_task, const uint64_t *d_base,
                                              const PlanesGatherBatchMember *d_members, const void *work, void *out, uint32_t grid, hipStream_t stream)
{
  if (d_ranges == nullptr || ((uintptr_t)d_ranges & 7) != 0 || d_header == nullptr || d_first_task == nullptr || d_base == nullptr || d_members == nullptr ||
      ((uintptr_t)d_members & 7) != 0 || work == nullptr || ((uintptr_t)work & 15) != 0 || out == nullptr || ((uintptr_t)out & 15) != 0 || grid == 0 || grid > 0x7FFFFFFFu)
    return hipErrorInvalidValue;
  (void)hipGetLastError();
  k_planes_merge_batch_indirect<<<grid, kThreads, 0, stream>>>(d_ranges, d_header, d_first_task, d_base, d_members, (const uint8_t *)work, (uint8_t *)out);
  return hipGetLastError();
}

} // namespace hsrans
