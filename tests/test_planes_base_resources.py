"""Build-time guard for the byte-plane kernels that take a base: the compiler's resource report (csrc/build/hsrans_planes_base.remarks) lists
exactly the twenty-two kernels — per residue rule (delta: the XOR; diff: the zigzag difference) k_planes_split_*, k_planes_merge_* and
k_planes_merge_ranges_* for 2-, 4- and 8-byte elements and the two table-driven ones — and none of them uses scratch or LDS (the 8-byte ones
hold 32 dwords of elements, 32 of the base and 32 of planes)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
RULES = ("delta", "diff")
# (mangled: length-prefixed name, then the element size as a template argument, or the first parameter of a plain function)
KERNELS = {f"{kind}_{rule}{W}": f"{len(f'k_planes_{kind}_{rule}')}k_planes_{kind}_{rule}ILj{W}EE" for rule in RULES for kind in ("split", "merge", "merge_ranges") for W in (2, 4, 8)}
KERNELS.update({f"{kind}_{rule}_batch": f"{len(f'k_planes_{kind}_{rule}_batch')}k_planes_{kind}_{rule}_batchEPK" for rule in RULES for kind in ("split", "merge")})


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes_base")


def test_the_report_lists_exactly_the_new_kernels(kernels):
    assert len(kernels) == len(KERNELS) == 22, sorted(kernels)
    for mangled in KERNELS.values():
        kernel_remarks.one(kernels, NS + mangled)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_uses_scratch_or_lds(kernels, kernel):
    report = kernel_remarks.one(kernels, NS + KERNELS[kernel])
    assert report["ScratchSize [bytes/lane]"] == 0, report
    assert report["LDS Size [bytes/block]"] == 0, report
