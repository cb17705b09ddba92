// hsrans_planes_batch.hip — k_planes_split_batch, k_planes_merge_batch and k_planes_store_batch: the byte-plane kernels for many tensors in
// ONE launch (hsrans_*_device_planes_batch).  A table of PlanesBatchMember records in device memory drives each: a workgroup finds its
// member by a binary search over the records' first_task — the same on every lane, on scalar loads — and then does exactly what workgroup
// (blockIdx.x - first_task) of the member's single launch does (hsrans_planes.hip: 16 elements per lane through planes_shuffle.h, the last
// n % 16 elements byte by byte by the first lanes of the member's last workgroup).  W is read from the record: 2-, 4- and 8-byte members
// share a launch.  The store kernel is the same walk with nothing to shuffle: 16 bytes per lane, the tail byte by byte.
#include "hsrans_planes.h"
#include "planes_shuffle.h"

namespace hsrans
{
namespace
{
using namespace planes_detail;

// (the table walk — member_of, task_of, uni_ptr — and a task's lanes' work — split_lanes, merge_lanes — are planes_shuffle.h's, shared with
// hsrans_planes_base.hip)
template <uint32_t W>
__device__ __forceinline__ void split_task(const PlanesBatchMember *m)
{
  const Task t = task_of(m);
  const uint8_t *in = uni_ptr(m->elements);
  uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->plane[p]);
  split_lanes<W, RuleNone>(in, nullptr, planes, t.n, t.whole, t.lane, t.last);
}

template <uint32_t W>
__device__ __forceinline__ void merge_task(const PlanesBatchMember *m)
{
  const Task t = task_of(m);
  uint8_t *out = uni_ptr(m->elements);
  const uint8_t *planes[W];
#pragma unroll
  for (uint32_t p = 0; p < W; p++)
    planes[p] = uni_ptr(m->plane[p]);
  merge_lanes<W, RuleNone>(planes, nullptr, out, t.n, t.whole, t.lane, t.last);
}

// grid: the table's task total; count: its records
__global__ __launch_bounds__(kThreads) void k_planes_split_batch(const PlanesBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->W);
  if (W == 2)
    split_task<2>(m);
  else if (W == 4)
    split_task<4>(m);
  else if (W == 8)
    split_task<8>(m);
}

__global__ __launch_bounds__(kThreads) void k_planes_merge_batch(const PlanesBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesBatchMember *m = member_of(members, count, blockIdx.x);
  const uint32_t W = uni(m->W);
  if (W == 2)
    merge_task<2>(m);
  else if (W == 4)
    merge_task<4>(m);
  else if (W == 8)
    merge_task<8>(m);
}

// plane[0] -> elements, n bytes: not one byte past them
__global__ __launch_bounds__(kThreads) void k_planes_store_batch(const PlanesBatchMember *__restrict__ members, uint32_t count)
{
  const PlanesBatchMember *m = member_of(members, count, blockIdx.x);
  const Task t = task_of(m);
  const uint8_t *src = uni_ptr(m->plane[0]);
  uint8_t *dst = uni_ptr(m->elements);
  if (t.lane < t.whole)
  {
    uint32_t w[4];
    load16(src + t.lane * 16, w);
    store16(dst + t.lane * 16, w);
  }
  const uint32_t tail = (uint32_t)(t.n % 16);
  if (t.last && threadIdx.x < tail)
  {
    const uint64_t i = t.whole * 16 + threadIdx.x;
    dst[i] = src[i];
  }
}
} // namespace

hipError_t launch_planes_split_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  k_planes_split_batch<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

hipError_t launch_planes_merge_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  k_planes_merge_batch<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

hipError_t launch_planes_store_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream)
{
  if (!planes_table_ok(d_members, count, n_tasks))
    return hipErrorInvalidValue;
  k_planes_store_batch<<<n_tasks, kThreads, 0, stream>>>(d_members, count);
  return hipGetLastError();
}

} // namespace hsrans
