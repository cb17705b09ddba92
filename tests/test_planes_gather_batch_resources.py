"""Build-time guard for the batch range-merge kernel: the compiler's resource report (csrc/build/hsrans_planes_gather_batch.remarks) lists
exactly the one kernel — k_planes_merge_ranges_batch, which serves 2-, 4- and 8-byte members in one launch — and it neither spills to
scratch nor uses LDS (like the single call's kernels, it holds a block's elements and planes in registers)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
KERNEL = "27k_planes_merge_ranges_batchE"  # (mangled: length-prefixed name, then the argument types)


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_gather_batch")


def test_the_report_lists_exactly_the_one_kernel(kernels):
    assert len(kernels) == 1, sorted(kernels)
    assert next(iter(kernels)).startswith(NS + KERNEL), sorted(kernels)


def test_the_kernel_neither_spills_nor_uses_lds(kernels):
    (found,) = kernels.values()
    assert found["ScratchSize [bytes/lane]"] == 0, found
    assert found["LDS Size [bytes/block]"] == 0, found
