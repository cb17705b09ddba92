"""Build-time guard for hsrans_decode_device_gather_batch's kernels (k_gather_set<MODE, SHARED>), from the compiler's resource report as
tests/test_gather_resources.py reads it: the six instantiations of k_gather, none spills to scratch, and the shared-table ones keep <= 64
VGPRs and 8 waves per SIMD — the rule k_gather is held to.  The private-table instantiations (LDS bounds their occupancy, not registers)
are reported, not bounded."""
import re

from test_kernel_resources import _report


def _gather_set():
    out = {}
    for name, r in _report("hsrans_kernels").items():
        m = re.search(r"k_gather_setILi(\d)ELb([01])E", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


def test_instantiations():
    assert sorted(_gather_set()) == [(0, False), (1, False), (2, False), (3, True), (4, True), (5, True)]


def test_no_scratch():
    for key, r in _gather_set().items():
        assert r["ScratchSize [bytes/lane]"] == 0, (key, r)


def test_shared_table_occupancy():
    for key, r in _gather_set().items():
        print("k_gather_set<%d, %s>: %d VGPRs, %d waves/SIMD" % (key[0], str(key[1]).lower(), r["VGPRs"], r["Occupancy [waves/SIMD]"]))
        if key[1]:
            assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (key, r)
