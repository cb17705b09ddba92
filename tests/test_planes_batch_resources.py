"""Build-time guard for the multi-tensor byte-plane kernels: the compiler's resource report (csrc/build/hsrans_planes_batch.remarks) lists
exactly the three kernels — k_planes_split_batch, k_planes_merge_batch, k_planes_store_batch — and none of them spills to scratch (the
split and the merge hold the 8-byte body's 32 dwords of elements and 32 of planes in registers, whatever the member's element size)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
KERNELS = {kind: f"20k_planes_{kind}_batchE" for kind in ("split", "merge", "store")}  # (mangled: length-prefixed name, then the arguments)


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_batch")


def test_the_report_lists_exactly_the_three_kernels(kernels):
    assert len(kernels) == 3, sorted(kernels)
    for mangled in KERNELS.values():
        assert sum(name.startswith(NS + mangled) for name in kernels) == 1, (mangled, sorted(kernels))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_spills(kernels, kernel):
    found = [r for name, r in kernels.items() if name.startswith(NS + KERNELS[kernel])]
    assert len(found) == 1, (kernel, sorted(kernels))
    assert found[0]["ScratchSize [bytes/lane]"] == 0, found[0]
