// hsrans_planes.h — the streaming kernels of the byte-plane layer: elements of W bytes split into W byte planes and planes interleaved back
// into elements (hsrans_planes.hip), and the interleave of element ranges (hsrans_planes_gather.hip; with the ranges in device memory
// hsrans_planes_gather_indirect.hip; of many frames at once hsrans_planes_gather_batch.hip, and with those rows in device memory
// hsrans_planes_gather_batch_indirect.hip), and the forms of the split and the merges that XOR a base in or take the zigzag of the
// difference against it (hsrans_planes_base.hip; the XOR forms of the last three range merges hsrans_planes_gather_delta.hip).
// plane[p][i] = elements[i * W + p]; W is 2, 4 or 8.
#ifndef HSRANS_PLANES_H
#define HSRANS_PLANES_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hsrans_hip.h" // HSRANS_PACK_CHUNK
#include "hsrans_carve.h"

namespace hsrans
{

constexpr uint32_t kPlanesMax = 8;
// the most elements one launch takes: 16 per lane, 256 lanes per workgroup, fewer than 2^31 workgroups
constexpr uint64_t kPlanesMaxElements = (uint64_t)1 << 42;

struct PlanePtrs // (by value in the kernel arguments; entries >= W unused)
{
  uint8_t *p[kPlanesMax];
};
// what every launcher that takes them asks of them: W in {2, 4, 8}, planes 0 .. W - 1 set and 16-byte aligned
inline bool planes_ptrs_ok(uint32_t W, const PlanePtrs &planes)
{
  if (W != 2 && W != 4 && W != 8)
    return false;
  for (uint32_t p = 0; p < W; p++)
    if (planes.p[p] == nullptr || ((uintptr_t)planes.p[p] & 15) != 0)
      return false;
  return true;
}
// The launchers' step from W (planes_ptrs_ok has passed) to a kernel's template argument: f(std::integral_constant<uint32_t, W>), so that
// `[&](auto w) { k<w()><<<grid, 256, 0, stream>>>(...); }` is the whole dispatch.  hipcc takes a kernel launch inside a generic lambda (host
// and device pass both instantiate the three kernels from it), so no macro and no table of kernel pointers is needed.
template <typename F>
inline void planes_with_width(uint32_t W, F &&f)
{
  if (W == 2)
    f(std::integral_constant<uint32_t, 2>{});
  else if (W == 4)
    f(std::integral_constant<uint32_t, 4>{});
  else
    f(std::integral_constant<uint32_t, 8>{});
}

// What a tensor coded against a base leaves in its planes, the residue rule: in ^ base (hsrans_*_device_planes_delta), or the zigzag of
// the wrapped difference in - base of the elements read as little-endian unsigned integers (hsrans_*_device_planes_diff).  Looked at only
// where there is a base.
enum class PlanesRule : uint32_t
{
  kXor,
  kDiff
};

// asynchronous on `stream`; every pointer 16-byte aligned, n in 1..kPlanesMaxElements, W in {2, 4, 8} (hipErrorInvalidValue otherwise).
// base: null, or as many bytes as the elements: the planes hold the residue by `rule` — k_planes_split_delta and k_planes_merge_delta or
// k_planes_split_diff and k_planes_merge_diff (hsrans_planes_base.hip) instead of the plain kernels.  The
// merge's base may be `out` itself: the residue undone in place; any other overlap of the two is the caller's to refuse.
hipError_t launch_planes_split(uint32_t W, const void *in, const void *base, PlanesRule rule, uint64_t n, const PlanePtrs &planes, hipStream_t stream);
hipError_t launch_planes_merge(uint32_t W, const PlanePtrs &planes, const void *base, PlanesRule rule, uint64_t n, void *out, hipStream_t stream);

// ---- many tensors in one launch (hsrans_*_device_planes_batch): k_planes_split_batch, k_planes_merge_batch, k_planes_store_batch
// (hsrans_planes_batch.hip), each driven by a table of these records in device memory, one workgroup per task ----
// A member's tasks are the workgroups of its single launch — planes_tasks_of(n), the last one moving the n % 16 tail elements — and
// first_task is the exclusive prefix of them over the table: a workgroup finds its member as the last one with first_task <= its index.
// W may differ from member to member.  k_planes_store_batch copies: W is 1, plane[0] the n bytes read, `elements` where they go.
struct PlanesBatchMember
{
  uint8_t *elements;         // split: read; merge and store: written
  uint8_t *plane[kPlanesMax]; // split: written; merge and store: read (entries >= W unused)
  uint64_t n;                // elements (store: bytes)
  uint32_t W, first_task;
};
constexpr uint32_t planes_tasks_of(uint64_t n) // (host and device; n <= kPlanesMaxElements: at most 2^30)
{
  return n / 16 > 256 ? (uint32_t)((n / 16 + 255) / 256) : 1;
}
// asynchronous on `stream`, one kernel each, n_tasks workgroups (the table's task total, 1 .. 2^31 - 1); the table's pointers are the
// caller's to check: set, 16-byte aligned, W in {2, 4, 8} (store: 1), n in 1..kPlanesMaxElements (hipErrorInvalidValue: a null table, no
// member, a task total out of range — planes_table_ok, for the tables of either record type)
inline bool planes_table_ok(const void *d_members, uint32_t count, uint32_t n_tasks)
{
  return d_members != nullptr && ((uintptr_t)d_members & 7) == 0 && count != 0 && n_tasks >= count && n_tasks <= 0x7FFFFFFFu;
}
hipError_t launch_planes_split_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream);
hipError_t launch_planes_merge_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream);
hipError_t launch_planes_store_batch(const PlanesBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream);

// ---- many byte ranges into one arena in one launch (hsrans_pack_device, hsrans_planes_pack_device): k_pack (hsrans_planes_pack.hip) ----
// An item's `length` bytes at src go to dst, and the bytes from there up to up16(length) are written as zero; its tasks are the chunks of
// kPackChunk bytes of those up16(length) bytes, one workgroup each, and first_task is their exclusive prefix over the table.
// (HSRANS_PACK_CHUNK_BUILD: the chunk of a tuning build of the library, `make pack_variants`; such a library's hsrans_pack_tasks counts in
// its own chunk, not in the header's)
#ifdef HSRANS_PACK_CHUNK_BUILD
constexpr uint32_t kPackChunk = HSRANS_PACK_CHUNK_BUILD;
#else
constexpr uint32_t kPackChunk = HSRANS_PACK_CHUNK; // (include/hsrans_hip.h)
#endif
static_assert(kPackChunk >= 4096 && (kPackChunk & (kPackChunk - 1)) == 0, "a power of two, at least one round of a workgroup's 16-byte lanes");
struct PackItem
{
  const uint8_t *src; // 16-byte aligned; not one byte at or behind src + length is read
  uint8_t *dst;       // 16-byte aligned
  uint64_t length;    // > 0
  uint32_t first_task, reserved;
};
constexpr uint64_t pack_tasks_of(uint64_t length) // (host and device; length <= 2^64 - 16)
{
  return (((length + 15) & ~(uint64_t)15) + kPackChunk - 1) / kPackChunk;
}
// asynchronous on `stream`, one kernel, n_tasks workgroups (the table's task total, 1 .. 2^31 - 1); the table's records are the caller's
// to check (hipErrorInvalidValue: a null table, no item, a task total out of range)
hipError_t launch_pack(const PackItem *d_items, uint32_t count, uint32_t n_tasks, hipStream_t stream);

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
// bit p of work_mask is set, else the stored plane; every pointer 16-byte aligned (hipErrorInvalidValue otherwise).  base: null, or the
// whole base tensor (hsrans_decode_device_planes_gather_delta, _gather_diff): output element (element + dst_delta) is what `rule` makes of
// the planes' element and base element `element` — k_planes_merge_ranges_delta or k_planes_merge_ranges_diff (hsrans_planes_base.hip)
// instead of the plain kernel
hipError_t launch_planes_merge_ranges(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks, const void *base,
                                      PlanesRule rule, void *out, hipStream_t stream);

// ---- rows of many frames in one launch (hsrans_decode_device_planes_gather_batch): k_planes_merge_ranges_batch
// (hsrans_planes_gather_batch.hip) ----
// A task as above with its row's sub-slot distance and member (hsrans_planes_gather_batch_task, include/hsrans_hip.h): plane p of the
// window lies at work_pos + p * plane_step of the call's workspace where the member's plane p was coded
struct PlanesGatherBatchTask
{
  uint64_t src, work_pos, plane_step;
  int64_t dst_delta;
  uint32_t lo, hi, member, reserved;
};
// a member's record, in device memory for the lifetime of the gather set: stored[p] where plane p lies in the member's frame (bit p of
// coded_mask clear), unused where it was coded
struct PlanesGatherBatchMember
{
  const uint8_t *stored[kPlanesMax];
  uint32_t W, coded_mask;
};
// asynchronous on `stream`, one workgroup per task (1 .. 2^31 - 1 of them, in device memory); the tasks' members index d_members, whose
// records are the caller's to check (W in {2, 4, 8}, stored planes set and 16-byte aligned); work and out 16-byte aligned
// (hipErrorInvalidValue otherwise)
hipError_t launch_planes_merge_ranges_batch(const PlanesGatherBatchTask *d_tasks, uint32_t n_tasks, const PlanesGatherBatchMember *d_members, const void *work, void *out,
                                            hipStream_t stream);

// ---- the same for ranges in device memory (hsrans_decode_device_planes_gather_indirect): k_planes_cut, the set's indirect gather, then
// k_planes_merge_indirect (hsrans_planes_gather_indirect.hip) ----
struct PlanesRange // (hsrans_range: offset, length, dst_offset, in elements)
{
  uint64_t offset, length, dst_offset;
};
struct PlanesSetRow // (hsrans_member_range: a row of the set's gather)
{
  uint64_t offset, length, dst_offset;
  uint32_t member, reserved;
};
// The control workspace, in bytes from its start: a header of uint32 words — [kPlanesWsTotal] the merge's tasks, 0 where the call was refused;
// [kPlanesWsCount] the ranges in use; [kPlanesWsRows] the rows of the set's gather (its count word), 0 where refused — then
// first_task[0 .. max_count] (uint32, the exclusive prefix of the ranges' task counts and their total), base[max_count] (uint64, B_r),
// rows[max_count * elem_size] (PlanesSetRow; the first count * coded are in use) and, from `set` on, the workspace of the set's own call.
constexpr uint32_t kPlanesWsTotal = 0, kPlanesWsCount = 1, kPlanesWsRows = 2;
struct PlanesCutWs
{
  size_t first_task, base, rows, set;
};
inline PlanesCutWs planes_cut_ws(uint32_t W, uint32_t max_count) // (host: the kernels get pointers)
{
  Carve c;
  PlanesCutWs ws;
  c.take(256);
  ws.first_task = c.take(((size_t)max_count + 1) * 4);
  ws.base = c.take((size_t)max_count * 8);
  ws.rows = c.take((size_t)max_count * W * sizeof(PlanesSetRow));
  ws.set = c.close();
  return ws;
}
struct PlanesCutParams
{
  const PlanesRange *ranges; // device
  const uint32_t *count;     // device, or null: max_count
  uint32_t max_count, coded; // coded planes, the set's members in order: member k is plane (coded_planes >> 4 k) & 15
  uint32_t coded_planes;
  uint64_t elements, out_elements; // the tensor's elements; the output's (out_capacity / elem_size)
  uint64_t stride;                 // the workspace regions' distance: no sum of slots may exceed it
  uint32_t *header, *first_task;   // the control workspace's parts
  uint64_t *base;
  PlanesSetRow *rows;
  uint32_t *status; // the gather object's word: kStatusBadRange where the call is refused
};
// the workgroups of the merge: the most tasks the call can have, max_count + stride / 4096 (a range's tasks <= its slot / 4096 + 1, and the
// slots fit in stride), capped at the workgroups of 256 lanes the device holds at once; k_planes_merge_indirect strides over the tasks
uint32_t planes_merge_indirect_grid(uint32_t num_cus, uint32_t W, uint32_t max_count, uint64_t stride);
// asynchronous on `stream`, one kernel each, nothing else (capturable); hipErrorInvalidValue for what launch_planes_merge_ranges refuses
hipError_t launch_planes_cut(const PlanesCutParams &cp, hipStream_t stream);
hipError_t launch_planes_merge_indirect(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesRange *d_ranges, const uint32_t *d_header,
                                        const uint32_t *d_first_task, const uint64_t *d_base, uint32_t grid, void *out, hipStream_t stream);

// ---- rows of many frames in device memory (hsrans_decode_device_planes_gather_batch_indirect): k_planes_cut_batch, the set's indirect
// gather, then k_planes_merge_batch_indirect (hsrans_planes_gather_batch_indirect.hip) ----
// what the cut reads of a row's member, in device memory for the lifetime of the gather set beside the merge's records: one 16-byte load
struct alignas(16) PlanesCutBatchMember
{
  uint64_t elements;
  uint32_t coded_at;       // the member's first coded plane among the set's members
  uint16_t W, coded_mask;  // element size; bit p: plane p was coded
};
// The control workspace, in bytes from its start: the header's words as above ([kPlanesWsRows]: the count word of the set's call), then
// first_task[0 .. max_count] (uint32), base[max_count] (uint64, C_r), first_row[max_count] (uint32: where the row's gather rows begin),
// rows[max_count * max_elem_size] (PlanesSetRow; the first header[kPlanesWsRows] are in use) and, from `set` on, the workspace of the set's
// own call.
struct PlanesCutBatchWs
{
  size_t first_task, base, first_row, rows, set;
};
inline PlanesCutBatchWs planes_cut_batch_ws(uint32_t max_elem_size, uint32_t max_count) // (host: the kernels get pointers)
{
  Carve c;
  PlanesCutBatchWs ws;
  c.take(256);
  ws.first_task = c.take(((size_t)max_count + 1) * 4);
  ws.base = c.take((size_t)max_count * 8);
  ws.first_row = c.take((size_t)max_count * 4);
  ws.rows = c.take((size_t)max_count * max_elem_size * sizeof(PlanesSetRow));
  ws.set = c.close();
  return ws;
}
struct PlanesCutBatchParams
{
  const PlanesSetRow *ranges;          // device: the call's rows (hsrans_member_range, in elements)
  const uint32_t *count;               // device, or null: max_count
  const PlanesCutBatchMember *members; // device: the set's cut records
  uint32_t max_count, n_members;
  uint64_t out_capacity; // bytes
  uint64_t work_limit;   // no sum of W * slot may exceed it: work_bytes rounded down to 256, at most 2^48 (so that no sum in the cut wraps)
  uint32_t *header, *first_task, *first_row; // the control workspace's parts
  uint64_t *base;
  PlanesSetRow *rows;
  uint32_t *status; // the gather set object's word: kStatusBadRange where the call is refused
};
// the workgroups of the merge: the most tasks the call can have, max_count + work_bytes / (min_W * 4096) (a row's tasks <= its slot / 4096
// + 1, and the rows' W * slot fit in work_bytes), capped at the workgroups of 256 lanes the device holds at once;
// k_planes_merge_batch_indirect strides over the tasks
uint32_t planes_merge_batch_indirect_grid(uint32_t num_cus, uint32_t min_W, uint32_t max_count, uint64_t work_bytes);
// asynchronous on `stream`, one kernel each, nothing else (capturable); hipErrorInvalidValue for a null or misaligned pointer or grid 0
hipError_t launch_planes_cut_batch(const PlanesCutBatchParams &cp, hipStream_t stream);
hipError_t launch_planes_merge_batch_indirect(const PlanesSetRow *d_ranges, const uint32_t *d_header, const uint32_t *d_first_task, const uint64_t *d_base,
                                              const PlanesGatherBatchMember *d_members, const void *work, void *out, uint32_t grid, hipStream_t stream);

// ---- tensors coded against a base (hsrans_*_device_planes_delta, hsrans_*_device_planes_diff): hsrans_planes_base.hip, the kernels of
// both residue rules.  The one-tensor launchers are the plain ones above, given a base; what that unit adds to them is the launch of its
// kernels alone, picked by `rule` — arguments checked and grid formed by the caller, nothing returned: the caller asks hipGetLastError ----
void planes_base_split_kernel(PlanesRule rule, uint32_t W, uint32_t grid, const uint8_t *in, const uint8_t *base, uint64_t n, const PlanePtrs &planes, hipStream_t stream);
void planes_base_merge_kernel(PlanesRule rule, uint32_t W, uint32_t grid, const PlanePtrs &planes, const uint8_t *base, uint64_t n, uint8_t *out, hipStream_t stream);
void planes_base_merge_ranges_kernel(PlanesRule rule, uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesGatherTask *d_tasks, uint32_t n_tasks,
                                     const uint8_t *base, uint8_t *out, hipStream_t stream);
// a PlanesBatchMember and the member's base; null: the member is split or merged as it is
struct PlanesDeltaBatchMember
{
  PlanesBatchMember m;
  const uint8_t *base;
};
// launch_planes_split_batch's and _merge_batch's contracts, over these records and under `rule`
hipError_t launch_planes_split_base_batch(PlanesRule rule, const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream);
hipError_t launch_planes_merge_base_batch(PlanesRule rule, const PlanesDeltaBatchMember *d_members, uint32_t count, uint32_t n_tasks, hipStream_t stream);

// ---- the gathers that undo a delta while they fetch (hsrans_decode_device_planes_gather_indirect_delta, _gather_batch_delta,
// _gather_batch_indirect_delta): hsrans_planes_gather_delta.hip.  Each launcher is its plain twin's above — the same arguments, the same
// checks — with the base: xbase, the whole base tensor in the frame's element coordinates (set and 16-byte aligned), or d_xbases, one base
// address per member of d_members in device memory, 0 for a member that goes as it is (the table set and 8-byte aligned; its entries are
// the caller's to check: 16-byte aligned, elem_size * elements bytes, clear of everything the call writes).  Output element
// (element + dst_delta) is XORed with base element `element`.  The cuts, task lists and control workspaces are the plain calls'. ----
// the workgroups of the two indirect merges: the plain grid functions' formula for the most tasks, capped by what the device holds of the
// DELTA kernels, which keep more registers than the plain ones
uint32_t planes_merge_indirect_delta_grid(uint32_t num_cus, uint32_t W, uint32_t max_count, uint64_t stride);
uint32_t planes_merge_batch_indirect_delta_grid(uint32_t num_cus, uint32_t min_W, uint32_t max_count, uint64_t work_bytes);
hipError_t launch_planes_merge_indirect_delta(uint32_t W, const PlanePtrs &planes, uint32_t work_mask, const PlanesRange *d_ranges, const uint32_t *d_header,
                                              const uint32_t *d_first_task, const uint64_t *d_base, const void *xbase, uint32_t grid, void *out, hipStream_t stream);
hipError_t launch_planes_merge_ranges_batch_delta(const PlanesGatherBatchTask *d_tasks, uint32_t n_tasks, const PlanesGatherBatchMember *d_members, const uint64_t *d_xbases,
                                                  const void *work, void *out, hipStream_t stream);
hipError_t launch_planes_merge_batch_indirect_delta(const PlanesSetRow *d_ranges, const uint32_t *d_header, const uint32_t *d_first_task, const uint64_t *d_base,
                                                    const PlanesGatherBatchMember *d_members, const uint64_t *d_xbases, const void *work, void *out, uint32_t grid,
                                                    hipStream_t stream);

} // namespace hsrans

#endif // HSRANS_PLANES_H
