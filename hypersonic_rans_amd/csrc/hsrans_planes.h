// hsrans_planes.h — the streaming kernels of the byte-plane layer: elements of W bytes split into W byte planes and planes interleaved back
// into elements (hsrans_planes.hip), and the interleave of element ranges (hsrans_planes_gather.hip).  plane[p][i] = elements[i * W + p];
// W is 2, 4 or 8.
#ifndef HSRANS_PLANES_H
#define HSRANS_PLANES_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace hsrans
{

constexpr uint32_t kPlanesMax = 8;
// the most elements one launch takes: 16 per lane, 256 lanes per workgroup, fewer than 2^31 workgroups
constexpr uint64_t kPlanesMaxElements = (uint64_t)1 << 42;

struct PlanePtrs // (by value in the kernel arguments; entries >= W unused)
{
  uint8_t *p[kPlanesMax];
};

// asynchronous on `stream`; every pointer 16-byte aligned, n in 1..kPlanesMaxElements, W in {2, 4, 8} (hipErrorInvalidValue otherwise)
hipError_t launch_planes_split(uint32_t W, const void *in, uint64_t n, const PlanePtrs &planes, hipStream_t stream);
hipError_t launch_planes_merge(uint32_t W, const PlanePtrs &planes, uint64_t n, void *out, hipStream_t stream);

// One workgroup's work of k_planes_merge_ranges (hsrans_planes_gather_task, include/hsrans_hip.h): the elements [src + lo, src + hi) of the
// tensor — src a multiple of 16, lo < 16, hi <= kPlanesGatherTaskElements — whose bytes lie at work_pos + (element - src) of a workspace region
// and at the element's own index of a stored plane, and go to output element (element + dst_delta)
constexpr uint32_t kPlanesGatherTaskElements = 4096;
struct PlanesGatherTask
{
  uint64_t src, work_pos;
  int64_t dst_delta;
  uint32_t lo, hi;
};
// asynchronous on `stream`, one workgroup per task (1 .. 2^31 - 1 of them, in device memory); planes.p[p]: plane p's workspace region where
// bit p of work_mask is set, else the stored plane; every pointer 16-byte aligned (hipErrorInvalidValue otherwise)
hipError_t launch_planes_merge_ranges(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks, void *out,
                                      hipStream_t stream);

} // namespace hsrans

#endif // HSRANS_PLANES_H
