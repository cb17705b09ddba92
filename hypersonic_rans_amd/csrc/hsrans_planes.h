// hsrans_planes.h — the two streaming kernels of the byte-plane layer (hsrans_planes.hip): elements of W bytes split into W byte planes, and
// planes interleaved back into elements.  plane[p][i] = elements[i * W + p]; W is 2, 4 or 8.
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

} // namespace hsrans

#endif // HSRANS_PLANES_H
