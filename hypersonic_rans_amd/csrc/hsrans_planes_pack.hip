// hsrans_planes_pack.hip — k_pack: many byte ranges into one arena in ONE launch (hsrans_pack_device, hsrans_planes_pack_device).  The shape
// of k_planes_store_batch (hsrans_planes_batch.hip), widened: a table of PackItem records in device memory drives it, a workgroup finds its
// item by the binary search over the records' first_task — the same on every lane, on scalar loads — and then moves chunk
// (blockIdx.x - first_task) of the item, kPackChunk bytes: kPackChunk / 4096 units of 16 bytes per lane, a workgroup's 256 lanes on
// neighbouring units, every load of a lane issued before its first store.  An item's last unit, where `length` is no multiple of 16, is
// read byte by byte — not one byte at or behind src + length — and completed with zeros: the arena's bytes are a pure function of the
// items' bytes.  Nothing outside [dst, dst + up16(length)) is written.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

// Non-temporal stores (the arena is written once and read by a later call): on 128 MiB of frames the pack took 0.7-7.0 us less with them than
// with plain ones at each chunk size (profiles/r23_planes_pack_variants.jsonl, CHANGELOG).  0: plain stores, for the variant builds of the
// Makefile's `pack_variants` (tools/planes_pack_rate.py --variant).
#ifndef HSRANS_PACK_NT
#define HSRANS_PACK_NT 1
#endif

namespace hsrans
{
namespace
{
using namespace planes_detail;

constexpr uint32_t kLaneUnits = kPackChunk / (kThreads * 16); // 16-byte units a lane moves
static_assert(kLaneUnits >= 1 && kLaneUnits * kThreads * 16 == kPackChunk, "a chunk is whole rounds of the workgroup's lanes");

// the item of task t: the last record with first_task <= t (first_task[0] is 0 and t is below the table's total); task_row's search
// (planes_shuffle.h) over a field of the records
__device__ __forceinline__ const PackItem *item_of(const PackItem *__restrict__ items, uint32_t count, uint32_t t)
{
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (uni(items[mid].first_task) <= t)
      lo = mid;
    else
      hi = mid;
  }
  return items + lo;
}

__device__ __forceinline__ void store16_arena(uint8_t *at, const uint32_t *w)
{
#if HSRANS_PACK_NT
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {w[0], w[1], w[2], w[3]};
  __builtin_nontemporal_store(v, (u32x4 *)at);
#else
  store16(at, w);
#endif
}

// grid: the table's task total; count: its records
__global__ __launch_bounds__(kThreads) void k_pack(const PackItem *__restrict__ items, uint32_t count)
{
  const PackItem *it = item_of(items, count, blockIdx.x);
  const uint8_t *src = global_at(uni64((uint64_t)it->src));
  uint8_t *dst = global_at(uni64((uint64_t)it->dst));
  const uint64_t length = uni64(it->length);
  const uint64_t base = (uint64_t)(blockIdx.x - uni(it->first_task)) * kPackChunk;

  uint32_t w[kLaneUnits][4];
#pragma unroll
  for (uint32_t j = 0; j < kLaneUnits; j++) // every whole unit of the lane first: all of its loads in flight at once
  {
    const uint64_t at = base + (uint64_t)(j * kThreads + threadIdx.x) * 16;
    if (at + 16 <= length)
      load16(src + at, w[j]);
  }
#pragma unroll
  for (uint32_t j = 0; j < kLaneUnits; j++) // the item's last unit (one lane of its last workgroup): its length - at bytes, then zeros
  {
    const uint64_t at = base + (uint64_t)(j * kThreads + threadIdx.x) * 16;
    if (at < length && at + 16 > length)
    {
      const uint32_t have = (uint32_t)(length - at);
      uint64_t lo = 0, hi = 0;
      for (uint32_t b = 0; b < have; b++)
      {
        const uint64_t v = src[at + b];
        if (b < 8)
          lo |= v << (8 * b);
        else
          hi |= v << (8 * (b - 8));
      }
      w[j][0] = (uint32_t)lo, w[j][1] = (uint32_t)(lo >> 32), w[j][2] = (uint32_t)hi, w[j][3] = (uint32_t)(hi >> 32);
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kLaneUnits; j++)
  {
    const uint64_t at = base + (uint64_t)(j * kThreads + threadIdx.x) * 16;
    if (at < length)
      store16_arena(dst + at, w[j]);
  }
}
} // namespace

hipError_t launch_pack(const PackItem *d_items, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (d_items == nullptr || ((uintptr_t)d_items & 7) != 0 || count == 0 || n_tasks < count || n_tasks > 0x7FFFFFFFu)
    return hipErrorInvalidValue;
  k_pack<<<n_tasks, kThreads, 0, stream>>>(d_items, count);
  return hipGetLastError();
}

} // namespace hsrans
