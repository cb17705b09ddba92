// planes_cut_batch.h — the rules of one ROW of hsrans_decode_device_planes_gather_batch, a range of one member among many, once for the host's
// cut (measure_rows, hsrans_capi_planes_gather_batch.cpp) and for the device's (k_planes_cut_batch, hsrans_planes_gather_batch_indirect.hip):
// the check of a row against its member, what it adds to the workspace (W * slot), its merge tasks and its rows of the set's gather; and the
// rule by which these add up over a call's rows.  A row's slot, task count and task k are planes_cut.h's, the one header included here.
// Host and device, no HIP header, no other project header, and it compiles with a plain host compiler (tests/test_planes_cut_batch.py).
// None of the checks forms a sum that can wrap.
#ifndef HSRANS_PLANES_CUT_BATCH_H
#define HSRANS_PLANES_CUT_BATCH_H

#include "planes_cut.h"

// What one row comes to: its slot in each of its member's W sub-slots, the W * slot bytes it takes of the workspace, its merge tasks and —
// one per coded plane of its member, none for an empty row — its rows of the set's gather.
struct PlanesRowCut
{
  uint64_t slot, work, tasks;
  uint32_t rows;
};

// an element size the layer has, as a shift: W = 2, 4 or 8 = 1 << planes_width_shift(W) (the rules below multiply and divide by shifting)
HSRANS_PLANES_CUT_FN bool planes_width_ok(uint32_t W) { return W == 2 || W == 4 || W == 8; }
HSRANS_PLANES_CUT_FN uint32_t planes_width_shift(uint32_t W) { return W == 2 ? 1 : W == 4 ? 2 : 3; }

// The row [offset, offset + length) of a member of `elements` elements of W bytes, `coded` of whose planes were coded: false where W is no
// element size, the row leaves the member or W * slot cannot be formed.  An empty row inside its member passes and comes to nothing.
HSRANS_PLANES_CUT_FN bool planes_row_cut(uint64_t offset, uint64_t length, uint64_t elements, uint32_t W, uint32_t coded, PlanesRowCut *cut)
{
  *cut = PlanesRowCut{0, 0, 0, 0};
  if (!planes_width_ok(W) || !planes_source_ok(offset, length, elements))
    return false;
  const uint32_t shift = planes_width_shift(W);
  cut->slot = planes_range_slot(offset, length);
  if (cut->slot > ~(uint64_t)0 >> shift)
    return false;
  cut->work = cut->slot << shift;
  cut->tasks = planes_range_tasks(offset, length);
  cut->rows = length != 0 ? coded : 0;
  return true;
}

// ... and its destination inside the output's out_capacity bytes: (dst_offset + length) * W <= out_capacity, no product formed
HSRANS_PLANES_CUT_FN bool planes_row_dest_ok(uint64_t dst_offset, uint64_t length, uint32_t W, uint64_t out_capacity)
{
  return planes_width_ok(W) && planes_dest_ok(dst_offset, length, out_capacity >> planes_width_shift(W));
}

// The rows of a call so far; `work` is C_r of the next row.
struct PlanesRowsSum
{
  uint64_t work, tasks, rows;
};
// one more row: false where the workspace's bytes wrap or the tasks or the gather rows reach kPlanesCutLimit (the sum is then undefined)
HSRANS_PLANES_CUT_FN bool planes_rows_add(PlanesRowsSum *sum, const PlanesRowCut &cut)
{
  if (cut.work > ~(uint64_t)0 - sum->work)
    return false;
  sum->work += cut.work;
  sum->tasks += cut.tasks; // (below 2^31 + 2^60 / 4096 + 1: no wrap)
  sum->rows += cut.rows;
  return sum->tasks < kPlanesCutLimit && sum->rows < kPlanesCutLimit;
}

#endif // HSRANS_PLANES_CUT_BATCH_H
