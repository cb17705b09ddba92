"""Build-time guard for hsrans_decode_device_gather_indirect's kernels (k_gather_cut, k_gather_ranges<MODE, SHARED>), from the
compiler's resource report as tests/test_gather_resources.py reads it: the six instantiations of k_gather's table layouts exist, none
spills to scratch, and the shared-table ones keep <= 64 VGPRs and 8 waves per SIMD — the rule k_gather is held to."""
import re

from test_kernel_resources import _report


def _ranges():
    out = {}
    for name, r in _report("hsrans_kernels").items():
        m = re.search(r"k_gather_rangesILi(\d)ELb([01])E", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


def _cut():
    return [r for name, r in _report("hsrans_kernels").items() if "k_gather_cut" in name]


def test_instantiations():
    assert sorted(_ranges()) == [(0, False), (1, False), (2, False), (3, True), (4, True), (5, True)]
    assert len(_cut()) == 1


def test_no_scratch():
    for key, r in _ranges().items():
        assert r["ScratchSize [bytes/lane]"] == 0, (key, r)
    assert _cut()[0]["ScratchSize [bytes/lane]"] == 0, _cut()


def test_shared_table_occupancy():
    for key, r in _ranges().items():
        print("k_gather_ranges<%d, %s>: %d VGPRs, %d waves/SIMD" % (key[0], str(key[1]).lower(), r["VGPRs"], r["Occupancy [waves/SIMD]"]))
        if key[1]:
            assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (key, r)
