"""Build-time guard for hsrans_decode_device_gather's kernels (k_gather<MODE, SHARED>), from the compiler's resource report as
tests/test_kernel_resources.py reads it: none spills to scratch, and the shared-table instantiations keep <= 64 VGPRs and 8 waves per
SIMD — the rule the shared-table decode kernels are held to, for the same reasons (16-wave workgroups, two per CU).  The private-table
instantiations (a table per wave: LDS bounds their occupancy, not registers) are reported, not bounded."""
import re

from test_kernel_resources import _report


def _gather():
    out = {}
    for name, r in _report("hsrans_kernels").items():
        m = re.search(r"k_gatherILi(\d)ELb([01])E", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


def test_instantiations():
    assert sorted(_gather()) == [(0, False), (1, False), (2, False), (3, True), (4, True), (5, True)]


def test_no_scratch():
    for key, r in _gather().items():
        assert r["ScratchSize [bytes/lane]"] == 0, (key, r)


def test_shared_table_occupancy():
    for key, r in _gather().items():
        print("k_gather<%d, %s>: %d VGPRs, %d waves/SIMD" % (key[0], str(key[1]).lower(), r["VGPRs"], r["Occupancy [waves/SIMD]"]))
        if key[1]:
            assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (key, r)
