"""Build-time guard for the kernels of the delta gathers: the compiler's resource report (csrc/build/hsrans_planes_gather_delta.remarks)
lists exactly the five kernels — k_planes_merge_indirect_delta for 2-, 4- and 8-byte elements, k_planes_merge_ranges_batch_delta and
k_planes_merge_batch_indirect_delta — and none of them uses scratch or LDS (the 8-byte bodies hold 32 dwords of elements, 32 of the base and
32 of planes).  The two indirect merges stride over their tasks on a grid sized from the waves a SIMD holds of them
(planes_merge_indirect_delta_grid, planes_merge_batch_indirect_delta_grid: a workgroup is one wave per SIMD, so a CU holds that many
workgroups): the constants in the source may not exceed what the report says of each kernel."""
import os
import re

import pytest

import kernel_remarks
from kernel_remarks import CSRC

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument, or the first parameter of a plain function)
KERNELS = {f"merge_indirect_delta{W}": f"{len('k_planes_merge_indirect_delta')}k_planes_merge_indirect_deltaILj{W}EE" for W in (2, 4, 8)}
KERNELS.update({kind: f"{len('k_planes_' + kind)}k_planes_{kind}EPK" for kind in ("merge_ranges_batch_delta", "merge_batch_indirect_delta")})


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_gather_delta")


def _constant(name, used_as):
    """a waves-per-SIMD constant of the unit's grid functions, read from its source"""
    text = open(os.path.join(CSRC, "hsrans_planes_gather_delta.hip")).read()
    m = re.search(rf"constexpr uint32_t {name} = (\d+);", text)
    assert m and used_as in text, name
    return int(m.group(1))


def test_the_report_lists_exactly_the_five_kernels(kernels):
    assert len(kernels) == len(KERNELS) == 5, sorted(kernels)
    for mangled in KERNELS.values():
        kernel_remarks.one(kernels, NS + mangled)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_uses_scratch_or_lds(kernels, kernel):
    report = kernel_remarks.one(kernels, NS + KERNELS[kernel])
    assert report["ScratchSize [bytes/lane]"] == 0, report
    assert report["LDS Size [bytes/block]"] == 0, report


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_single_indirect_merge_keeps_the_occupancy_its_grid_is_sized_from(kernels, W):
    report = kernel_remarks.one(kernels, NS + KERNELS[f"merge_indirect_delta{W}"])
    waves = _constant(f"kMergeIndirectDeltaWavesPerSimd{W}", f"{':' if W == 8 else '?'} kMergeIndirectDeltaWavesPerSimd{W}")  # (its place in the grid function)
    assert 1 <= waves <= report["Occupancy [waves/SIMD]"], report


def test_the_batch_indirect_merge_keeps_the_occupancy_its_grid_is_sized_from(kernels):
    report = kernel_remarks.one(kernels, NS + KERNELS["merge_batch_indirect_delta"])
    waves = _constant("kMergeBatchIndirectDeltaWavesPerSimd", "* kMergeBatchIndirectDeltaWavesPerSimd")
    assert 1 <= waves <= report["Occupancy [waves/SIMD]"], report
