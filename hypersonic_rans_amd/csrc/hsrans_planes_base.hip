// hsrans_planes_base.hip — the byte-plane kernels for a tensor coded against a base, under either residue rule (planes_shuffle.h states
// them): the XOR (hsrans_*_device_planes_delta, RuleXor, the `_delta` kernels) and the zigzag of the wrapped difference
// (hsrans_*_device_planes_diff, RuleDiff, the `_diff` kernels).  Per rule: k_planes_split_*<W> and k_planes_merge_*<W> are k_planes_split
// and k_planes_merge (hsrans_planes.hip) with the lane's 16 W base bytes loaded beside its 16 W element bytes — one more 16-byte load per
// 16 bytes moved; k_planes_split_*_batch and k_planes_merge_*_batch are the table-driven forms (hsrans_planes_batch.hip) whose records
// carry a base pointer, null for a member that is coded as it is (RuleNone); k_planes_merge_ranges_*<W> is k_planes_merge_ranges
// (hsrans_planes_gather.hip) with the base read at the SOURCE element's index.
// Everything but three kernel templates is one statement over split_lanes / merge_lanes (planes_shuffle.h) and the table walk below.
// k_planes_merge_delta<W> has merge_lanes written out, and the two range merges have k_planes_merge_ranges' block body in a copy each
// (planes_shuffle.h says why, for both).
// In place.  The whole-tensor merges take out == base: neither is __restrict__, and the order that makes it safe is merge_lanes' (stated
// there).  Partial overlap is not safe, and the entries refuse it.
// No LDS, no scratch.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

namespace hsrans
{
namespace
{
using namespace planes_detail;

// ---- one tensor: the grids of hsrans_planes.hip, the lanes' work with a base ----
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_split_delta(const uint8_t *__restrict__ in, const uint8_t *__restrict__ base, uint64_t n, PlanePtrs planes)
{
  split_lanes<W, RuleXor>(in, base, planes.p, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_split_diff(const uint8_t *__restrict__ in, const uint8_t *__restrict__ base, uint64_t n, PlanePtrs planes)
{
  split_lanes<W, RuleDiff>(in, base, planes.p, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}

// merge_lanes<W, RuleXor> written out, like k_planes_merge<W> (hsrans_planes.hip) and for its reason: as a call to it the kernel reads all
// its arguments on entry and at W = 4 took 85.6 against 84.6 µs on 128 MiB (medians of 96, three rounds; 124.7 against 123.9 in place).
// (base and out may be the same buffer: not __restrict__, all base loads of a lane before its first store, the tail's base byte read and
// then written — merge_lanes' order, planes_shuffle.h)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_delta(PlanePtrs planes, const uint8_t *base, uint64_t n, uint8_t *out)
{
  const uint64_t whole = n / kLaneElements, lane = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (lane < whole)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(planes.p[p] + lane * kLaneElements, pl[p]);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(base + lane * (kLaneElements * W) + 16 * k, b + 4 * k);
    merge16<W>(pl, e);
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
      e[k] ^= b[k];
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      store16(out + lane * (kLaneElements * W) + 16 * k, e + 4 * k);
  }
  const uint32_t tail = (uint32_t)(n % kLaneElements);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x < tail)
  {
    const uint64_t i = whole * kLaneElements + threadIdx.x;
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
    {
      const uint8_t b = base[i * W + p];
      out[i * W + p] = planes.p[p][i] ^ b;
    }
  }
}
// (base and out may be the same buffer: not __restrict__)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_diff(PlanePtrs planes, const uint8_t *base, uint64_t n, uint8_t *out)
{
  merge_lanes<W, RuleDiff>(planes.p, base, out, n, n / kLaneElements, (uint64_t)blockIdx.x * kThreads + threadIdx.x, blockIdx.x == gridDim.x - 1);
}

// ---- many tensors: the table walk of hsrans_planes_batch.hip (member_of, task_of, uni_ptr: planes_shuffle.h) over records with a base ----
template <uint32_t W, typename Rule>
__device__ __forceinline__ void split_task(const PlanesDeltaBatchMember *m)
{
  const Task t = task_of(&m->m);
  const uint8_t *in = uni_ptr(m->m.elements), *base = uni_ptr(m->base);
  uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->m.plane[p]);
  split_lanes<W, Rule>(in, base, planes, t.n, t.whole, t.lane, t.last);
}

template <uint32_t W, typename Rule>
__device__ __forceinline__ void merge_task(const PlanesDeltaBatchMember *m)
{
  const Task t = task_of(&m->m);
  uint8_t *out = uni_ptr(m->m.elements);
  const uint8_t *base = uni_ptr(m->base); // (may be `out`)
  const uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->m.plane[p]);
  merge_lanes<W, Rule>(planes, base, out, t.n, t.whole, t.lane, t.last);
}

template <typename Rule>
__device__ __forceinline__ void split_member(const PlanesDeltaBatchMember *m, uint32_t W)
{
  if (W == 2)
    split_task<2, Rule>(m);
  else if (W == 4)
    split_task<4, Rule>(m);
  else if (W == 8)
    split_task<8, Rule>(m);
}
template <typename Rule>
__device__ __forceinline__ void merge_member(const PlanesDeltaBatchMember *m, uint32_t W)
{
  if (W == 2)
    merge_task<2, Rule>(m);
  else if (W == 4)
    merge_task<4, Rule>(m);
  else if (W == 8)
    merge_task<8, Rule>(m);
}

// a workgroup's member of the table; whether it has a base is decided per workgroup, from the record: without one it takes RuleNone
template <typename Rule>
__device__ __forceinline__ void split_table(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesDeltaBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->m.W);
  if (uni64((uint64_t)m->base) != 0)
    split_member<Rule>(m, W);
  else
    split_member<RuleNone>(m, W);
}
template <typename Rule>
__device__ __forceinline__ void merge_table(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesDeltaBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->m.W);
  if (uni64((uint64_t)m->base) != 0)
    merge_member<Rule>(m, W);
  else
    merge_member<RuleNone>(m, W);
}

// grid: the table's task total; count: its records
__global__ __launch_bounds__(kThreads) void k_planes_split_delta_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count) { split_table<RuleXor>(members, count); }
__global__ __launch_bounds__(kThreads) void k_planes_merge_delta_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count) { merge_table<RuleXor>(members, count); }
__global__ __launch_bounds__(kThreads) void k_planes_split_diff_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count) { split_table<RuleDiff>(members, count); }
__global__ __launch_bounds__(kThreads) void k_planes_merge_diff_batch(const PlanesDeltaBatchMember *__restrict__ members, uint32_t count) { merge_table<RuleDiff>(members, count); }

// ---- element ranges of one frame: k_planes_merge_ranges' body (hsrans_planes_gather.hip) with the base, a copy per rule (planes_shuffle.h) ----
static_assert(kThreads * kLaneElements == kPlanesGatherTaskElements, "one lane per 16-element block of a task");

// grid: one workgroup per task; xbase: the whole base tensor, in the frame's element coordinates (never the output: __restrict__)
template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges_delta(PlanePtrs planes, uint32_t work_mask, const PlanesGatherTask *__restrict__ tasks,
                                                                        const uint8_t *__restrict__ xbase, uint8_t *__restrict__ out)
{
  const PlanesGatherTask t = tasks[blockIdx.x];
  const uint32_t first = threadIdx.x * kLaneElements; // the lane's block: elements [src + first, src + first + 16)
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements; // (t.lo < 16: only lane 0 has a head)
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    src[p] = planes.p[p] + (((work_mask >> p) & 1) != 0 ? t.work_pos : t.src) + first;
  const uint8_t *bsrc = xbase + (t.src + first) * W; // the block's base bytes: 16-byte aligned (src a multiple of 16 elements)
  const uint64_t base = t.src + first + (uint64_t)t.dst_delta; // the output element of the block's element 0 (modulo 2^64: a head's may lie below 0)
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(bsrc + 16 * k, b + 4 * k);
    merge16<W>(pl, e);
#pragma unroll
    for (uint32_t k = 0; k < 4 * W; k++)
      e[k] ^= b[k];
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
  for (uint32_t i = lo; i < hi; i++) // (base bytes of the range's own elements only)
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      out[(base + i) * W + p] = src[p][i] ^ bsrc[i * W + p];
}

template <uint32_t W>
__global__ __launch_bounds__(kThreads) void k_planes_merge_ranges_diff(PlanePtrs planes, uint32_t work_mask, const PlanesGatherTask *__restrict__ tasks,
                                                                       const uint8_t *__restrict__ xbase, uint8_t *__restrict__ out)
{
  const PlanesGatherTask t = tasks[blockIdx.x];
  const uint32_t first = threadIdx.x * kLaneElements;
  if (first >= t.hi)
    return;
  const uint32_t lo = first < t.lo ? t.lo - first : 0, hi = t.hi - first < kLaneElements ? t.hi - first : kLaneElements;
  const uint8_t *src[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    src[p] = planes.p[p] + (((work_mask >> p) & 1) != 0 ? t.work_pos : t.src) + first;
  const uint8_t *bsrc = xbase + (t.src + first) * W;
  const uint64_t base = t.src + first + (uint64_t)t.dst_delta;
  if (lo == 0 && hi == kLaneElements)
  {
    uint32_t e[4 * W], b[4 * W], pl[W][4];
#pragma unroll
    for (uint32_t p = 0; p < W; p++)
      load16(src[p], pl[p]);
#pragma unroll
    for (uint32_t k = 0; k < W; k++)
      load16(bsrc + 16 * k, b + 4 * k);
    merge16<W>(pl, e);
    undiff_words<W>(e, b);
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
  for (uint32_t i = lo; i < hi; i++) // (base elements of the range's own elements only)
    *(typename ElementOf<W>::type *)(out + (base + i) * W) = undo_zigzag(z_at<W>(src, i), element_at<W>(bsrc, i));
}

} // namespace

// ---- the launches alone: launch_planes_split, _merge and _merge_ranges check the arguments and form the grid, and come here with a base
// and its rule; the kernel is picked per element size, by the rule ----
void planes_base_split_kernel(PlanesRule rule, uint32_t W, uint32_t grid, const uint8_t *in, const uint8_t *base, uint64_t n, const PlanePtrs &planes, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) {
    const auto kernel = rule == PlanesRule::kDiff ? k_planes_split_diff<w()> : k_planes_split_delta<w()>;
    kernel<<<grid, kThreads, 0, stream>>>(in, base, n, planes);
  });
}

void planes_base_merge_kernel(PlanesRule rule, uint32_t W, uint32_t grid, const PlanePtrs &planes, const uint8_t *base, uint64_t n, uint8_t *out, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) {
    const auto kernel = rule == PlanesRule::kDiff ? k_planes_merge_diff<w()> : k_planes_merge_delta<w()>;
    kernel<<<grid, kThreads, 0, stream>>>(planes, base, n, out);
  });
}

void planes_base_merge_ranges_kernel(PlanesRule rule, uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks,
                                     const uint8_t *base, uint8_t *out, hipStream_t stream)
{
  planes_with_width(W, [&](auto w) {
    const auto kernel = rule == PlanesRule::kDiff ? k_planes_merge_ranges_diff<w()> : k_planes_merge_ranges_delta<w()>;
    kernel<<<n_tasks, kThreads, 0, stream>>>(planes, work_mask, d_tasks, base, out);
  });
}

hipError_t launch_planes_split_base_batch(PlanesRule rule, const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  const auto kernel = rule == PlanesRule::kDiff ? k_planes_split_diff_batch : k_planes_split_delta_batch;
  kernel<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

hipError_t launch_planes_merge_base_batch(PlanesRule rule, const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  const auto kernel = rule == PlanesRule::kDiff ? k_planes_merge_diff_batch : k_planes_merge_delta_batch;
  kernel<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

} // namespace hsrans
