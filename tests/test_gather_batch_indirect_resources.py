"""Build-time guard for hsrans_decode_device_gather_batch_indirect's kernels — k_set_cut and k_set_ranges — from the compiler's resource
report as tests/test_kernel_resources.py reads it: k_set_ranges has its six instantiations <MODE, SHARED>, none spills to scratch, the
shared-table ones keep <= 64 VGPRs and 8 waves per SIMD (the rule of tests/test_gather_resources.py, for the same reasons), and there is
exactly one k_set_cut, without scratch.  The private-table instantiations are reported, not bounded."""
import re

from test_kernel_resources import _report


def _ranges():
    out = {}
    for name, r in _report("hsrans_kernels").items():
        m = re.search(r"k_set_rangesILi(\d)ELb([01])E", name)
        if m:
            out[(int(m.group(1)), m.group(2) == "1")] = r
    return out


def test_instantiations():
    assert sorted(_ranges()) == [(0, False), (1, False), (2, False), (3, True), (4, True), (5, True)]


def test_no_scratch():
    for key, r in _ranges().items():
        assert r["ScratchSize [bytes/lane]"] == 0, (key, r)


def test_shared_table_occupancy():
    shared = 0
    for key, r in _ranges().items():
        print("k_set_ranges<%d, %s>: %d VGPRs, %d waves/SIMD" % (key[0], str(key[1]).lower(), r["VGPRs"], r["Occupancy [waves/SIMD]"]))
        if key[1]:
            shared += 1
            assert r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, (key, r)
    assert shared == 3


def test_cut_kernel():
    cut = [r for name, r in _report("hsrans_kernels").items() if "k_set_cut" in name]
    assert len(cut) == 1 and cut[0]["ScratchSize [bytes/lane]"] == 0, cut


def test_names_leave_the_other_families_alone():
    """tests/test_gather_resources.py and tests/test_kernel_resources.py find their kernels by name"""
    for name in _report("hsrans_kernels"):
        if "k_set_cut" in name or "k_set_ranges" in name:
            for other in ("k_gather_cut", "k_gather_set", "k_gather_ranges", "k_decode_batch", "k_decode_spread", "k_decode_persist"):
                assert other not in name, name
