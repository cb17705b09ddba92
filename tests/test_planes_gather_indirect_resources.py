"""Build-time guard for the kernels of hsrans_decode_device_planes_gather_indirect: the compiler's resource report
(csrc/build/hsrans_planes_gather_indirect.remarks) lists exactly k_planes_cut and k_planes_merge_indirect for 2-, 4- and 8-byte elements; none
spills to scratch; the merge kernels use no LDS and keep the waves per SIMD the merge's grid is sized from (planes_merge_indirect_grid: a
workgroup is one wave per SIMD, so a CU holds that many workgroups)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument)
CUT = "12k_planes_cutE"
MERGE = {f"W{W}": f"23k_planes_merge_indirectILj{W}EE" for W in (2, 4, 8)}
WAVES_PER_SIMD = {"W2": 8, "W4": 8, "W8": 7}


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_gather_indirect")


def _one(kernels, mangled):
    return kernel_remarks.one(kernels, NS + mangled)


def test_the_report_lists_exactly_the_four_kernels(kernels):
    assert len(kernels) == 4, sorted(kernels)
    for mangled in [CUT[:-1]] + list(MERGE.values()):
        _one(kernels, mangled)


def test_the_cut_does_not_spill(kernels):
    assert _one(kernels, CUT[:-1])["ScratchSize [bytes/lane]"] == 0


@pytest.mark.parametrize("kernel", sorted(MERGE))
def test_the_merge_neither_spills_nor_uses_lds_and_keeps_its_occupancy(kernels, kernel):
    r = _one(kernels, MERGE[kernel])
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] == 0, r
    assert r["Occupancy [waves/SIMD]"] >= WAVES_PER_SIMD[kernel], r
