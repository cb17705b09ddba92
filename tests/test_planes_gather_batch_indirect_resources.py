"""Build-time guard for the kernels of hsrans_decode_device_planes_gather_batch_indirect: the compiler's resource report
(csrc/build/hsrans_planes_gather_batch_indirect.remarks) lists exactly k_planes_cut_batch and k_planes_merge_batch_indirect; neither spills to
scratch; the merge — one kernel for 2-, 4- and 8-byte members — uses no LDS and keeps the waves per SIMD its grid is sized from
(planes_merge_batch_indirect_grid: a workgroup is one wave per SIMD, so a CU holds that many workgroups)."""
import os
import re

import pytest

import kernel_remarks
from kernel_remarks import CSRC

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the argument types)
CUT = "18k_planes_cut_batchE"
MERGE = "29k_planes_merge_batch_indirectE"


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_gather_batch_indirect")


def _one(kernels, mangled):
    return kernel_remarks.one(kernels, NS + mangled)


def _grid_constant():
    """the waves per SIMD planes_merge_batch_indirect_grid multiplies the compute units by, read from the unit's source"""
    text = open(os.path.join(CSRC, "hsrans_planes_gather_batch_indirect.hip")).read()
    m = re.search(r"constexpr uint32_t kMergeBatchIndirectWavesPerSimd = (\d+);", text)
    assert m and "* kMergeBatchIndirectWavesPerSimd" in text
    return int(m.group(1))


def test_the_report_lists_exactly_the_two_kernels(kernels):
    assert len(kernels) == 2, sorted(kernels)
    _one(kernels, CUT)
    _one(kernels, MERGE)


def test_the_cut_does_not_spill(kernels):
    assert _one(kernels, CUT)["ScratchSize [bytes/lane]"] == 0


def test_the_merge_neither_spills_nor_uses_lds_and_keeps_its_occupancy(kernels):
    r = _one(kernels, MERGE)
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] == 0, r
    assert _grid_constant() == 8
    assert r["Occupancy [waves/SIMD]"] >= _grid_constant(), r
