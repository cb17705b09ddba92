"""Build-time guard for the kernels of hsrans_decode_device_planes_gather_batch_indirect: the compiler's resource report
(csrc/build/hsrans_planes_gather_batch_indirect.remarks) lists exactly k_planes_cut_batch and k_planes_merge_batch_indirect; neither spills to
scratch; the merge — one kernel for 2-, 4- and 8-byte members — uses no LDS and keeps the waves per SIMD its grid is sized from
(planes_merge_batch_indirect_grid: a workgroup is one wave per SIMD, so a CU holds that many workgroups)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
BUILD = os.path.join(CSRC, "build")
NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the argument types)
CUT = "18k_planes_cut_batchE"
MERGE = "29k_planes_merge_batch_indirectE"


@pytest.fixture(scope="module")
def kernels():
    path = os.path.join(BUILD, "hsrans_planes_gather_batch_indirect.remarks")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    out, cur = {}, None
    for line in open(path).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _one(kernels, mangled):
    found = [r for name, r in kernels.items() if name.startswith(NS + mangled)]
    assert len(found) == 1, (mangled, sorted(kernels))
    return found[0]


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
