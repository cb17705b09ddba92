"""Build-time guard for the diff byte-plane kernels: the compiler's resource report (csrc/build/hsrans_planes_diff.remarks) lists exactly the
eleven kernels — k_planes_split_diff, k_planes_merge_diff and k_planes_merge_ranges_diff for 2-, 4- and 8-byte elements and the two
table-driven ones — and none of them uses scratch or LDS (the 8-byte ones hold 32 dwords of elements, 32 of the base and 32 of planes)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument, or the first parameter of a plain function)
KERNELS = {f"{kind}{W}": f"{len('k_planes_' + kind)}k_planes_{kind}ILj{W}EE" for kind in ("split_diff", "merge_diff", "merge_ranges_diff") for W in (2, 4, 8)}
KERNELS.update({kind: f"{len('k_planes_' + kind)}k_planes_{kind}EPK" for kind in ("split_diff_batch", "merge_diff_batch")})


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_diff")


def test_the_report_lists_exactly_the_new_kernels(kernels):
    assert len(kernels) == len(KERNELS) == 11, sorted(kernels)
    for mangled in KERNELS.values():
        kernel_remarks.one(kernels, NS + mangled)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_uses_scratch_or_lds(kernels, kernel):
    report = kernel_remarks.one(kernels, NS + KERNELS[kernel])
    assert report["ScratchSize [bytes/lane]"] == 0, report
    assert report["LDS Size [bytes/block]"] == 0, report
