"""Build-time guard for the gather kernels — k_gather (hsrans_decode_device_gather), k_gather_ranges and k_gather_cut
(hsrans_decode_device_gather_indirect), k_gather_set (hsrans_decode_device_gather_batch) — from the compiler's resource report as
tests/test_kernel_resources.py reads it: each family has its six instantiations <MODE, SHARED>, none spills to scratch, and the
shared-table instantiations keep <= 64 VGPRs and 8 waves per SIMD — the rule the shared-table decode kernels are held to, for the same
reasons (16-wave workgroups, two per CU).  The private-table instantiations (a table per wave: LDS bounds their occupancy, not
registers) are reported, not bounded."""
import re

import pytest

from test_kernel_resources import _report

FAMILIES = ("k_gather", "k_gather_ranges", "k_gather_set")
families = pytest.mark.parametrize("family", FAMILIES)


def _family(family):
    out = {}
    for name, r in _report("hsrans_kernels").items():
        m = re.search(family + r"ILi(\d)ELb([01])E", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


@families
def test_instantiations(family):
    assert sorted(_family(family)) == [(0, False), (1, False), (2, False), (3, True), (4, True), (5, True)]


@families
def test_no_scratch(family):
    for key, r in _family(family).items():
        assert r["ScratchSize [bytes/lane]"] == 0, (key, r)


@families
def test_shared_table_occupancy(family):
    for key, r in _family(family).items():
        print("%s<%d, %s>: %d VGPRs, %d waves/SIMD" % (family, key[0], str(key[1]).lower(), r["VGPRs"], r["Occupancy [waves/SIMD]"]))
        if key[1]:
            assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (key, r)


def test_cut_kernel():
    cut = [r for name, r in _report("hsrans_kernels").items() if "k_gather_cut" in name]
    assert len(cut) == 1 and cut[0]["ScratchSize [bytes/lane]"] == 0, cut
