"""Build-time guard for the range-merge kernels: the compiler's resource report (csrc/build/hsrans_planes_gather.remarks) lists exactly the
three kernels — k_planes_merge_ranges for 2-, 4- and 8-byte elements — and none of them spills to scratch or uses LDS (like the two
whole-frame kernels, they hold a block's elements and planes in registers)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument)
KERNELS = {f"W{W}": f"21k_planes_merge_rangesILj{W}EE" for W in (2, 4, 8)}


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_gather")


def test_the_report_lists_exactly_the_three_kernels(kernels):
    assert len(kernels) == 3, sorted(kernels)
    for mangled in KERNELS.values():
        assert sum(name.startswith(NS + mangled) for name in kernels) == 1, (mangled, sorted(kernels))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_spills_or_uses_lds(kernels, kernel):
    found = [r for name, r in kernels.items() if name.startswith(NS + KERNELS[kernel])]
    assert len(found) == 1, (kernel, sorted(kernels))
    assert found[0]["ScratchSize [bytes/lane]"] == 0, found[0]
    assert found[0]["LDS Size [bytes/block]"] == 0, found[0]
