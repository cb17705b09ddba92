// planes_cut.h — the rules of one element range of hsrans_decode_device_planes_gather, once for the host's cut (cut_ranges / measure_ranges,
// hsrans_capi_planes_gather.cpp) and for the device's (k_planes_cut, k_planes_merge_indirect: hsrans_planes_gather_indirect.hip): the check of
// a range, its slot in every plane's workspace region, its tasks, and task k of it.  Host and device, nothing else included: no HIP header,
// no other project header, and it compiles with a plain host compiler (tests/test_planes_cut.py).  None of the checks forms a sum that can wrap.
#ifndef HSRANS_PLANES_CUT_H
#define HSRANS_PLANES_CUT_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HSRANS_PLANES_CUT_FN __host__ __device__ __forceinline__
#else
#define HSRANS_PLANES_CUT_FN inline
#endif

constexpr uint64_t kPlanesCutTask = 4096; // elements of a task (kPlanesGatherTaskElements, hsrans_planes.h)
// what a call may come to: fewer merge tasks and fewer gather rows than this (a launch's workgroups, the set's limit)
constexpr uint64_t kPlanesCutLimit = (uint64_t)1 << 31;

// [offset, offset + length) lies inside [0, extent]: (extent, 0) passes, (extent + 1, 0) does not (gather_extent_ok's form, hsrans_kernels.h)
HSRANS_PLANES_CUT_FN bool planes_extent_ok(uint64_t offset, uint64_t length, uint64_t extent) { return offset <= extent && length <= extent - offset; }

// A range of the tensor's `elements` that the cut takes: inside the tensor, and its slot can be formed.  With phase = offset & 15 <= offset,
// phase + length <= offset + length <= elements cannot wrap once the extent holds; only the rounding up to 16 can.
HSRANS_PLANES_CUT_FN bool planes_source_ok(uint64_t offset, uint64_t length, uint64_t elements)
{
  return planes_extent_ok(offset, length, elements) && (offset & 15) + length <= ~(uint64_t)0 - 15;
}
// ... and its destination inside the output's out_elements = out_capacity / elem_size elements
HSRANS_PLANES_CUT_FN bool planes_dest_ok(uint64_t dst_offset, uint64_t length, uint64_t out_elements) { return planes_extent_ok(dst_offset, length, out_elements); }

// the slot of a range that passed planes_source_ok in every plane's region: up16(phase + length) bytes, none for an empty range
HSRANS_PLANES_CUT_FN uint64_t planes_range_slot(uint64_t offset, uint64_t length) { return length != 0 ? ((offset & 15) + length + 15) & ~(uint64_t)15 : 0; }

// ... and its tasks: windows of 4096 elements from the range's 16-element grid point A = offset - phase on
HSRANS_PLANES_CUT_FN uint64_t planes_range_tasks(uint64_t offset, uint64_t length) { return length != 0 ? ((offset & 15) + length - 1) / kPlanesCutTask + 1 : 0; }

// Task k < planes_range_tasks of a non-empty range whose slot begins at `base` (B_r): the window [A + 4096 k, A + 4096 (k + 1)) clipped to the
// range.  Task: {uint64 src, work_pos; int64 dst_delta; uint32 lo, hi} (hsrans_planes_gather_task, PlanesGatherTask).
template <typename Task>
HSRANS_PLANES_CUT_FN Task planes_task_at(uint64_t offset, uint64_t length, uint64_t dst_offset, uint64_t base, uint64_t k)
{
  const uint64_t phase = offset & 15, first = offset - phase, stop = offset + length, src = first + k * kPlanesCutTask;
  // (an aggregate in the fields' order: src, work_pos, dst_delta — modulo 2^64, the merge adds it back the same way —, lo, hi)
  return Task{src, base + k * kPlanesCutTask, (int64_t)(dst_offset - offset), k == 0 ? (uint32_t)phase : 0, (uint32_t)(stop - src < kPlanesCutTask ? stop - src : kPlanesCutTask)};
}

#endif // HSRANS_PLANES_CUT_H
