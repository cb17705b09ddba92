"""Build-time guard for the byte-plane kernels: the compiler's resource report (csrc/build/hsrans_planes.remarks) lists exactly the six
kernels — k_planes_split and k_planes_merge for 2-, 4- and 8-byte elements — and none of them spills to scratch (the 8-byte ones hold
32 dwords of elements and 32 of planes in registers)."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument)
KERNELS = {f"{kind}{W}": f"14k_planes_{kind}ILj{W}EE" for kind in ("split", "merge") for W in (2, 4, 8)}


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_planes")


def test_the_report_lists_exactly_the_six_kernels(kernels):
    assert len(kernels) == 6, sorted(kernels)
    for mangled in KERNELS.values():
        assert sum(name.startswith(NS + mangled) for name in kernels) == 1, (mangled, sorted(kernels))


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_kernel_spills(kernels, kernel):
    found = [r for name, r in kernels.items() if name.startswith(NS + KERNELS[kernel])]
    assert len(found) == 1, (kernel, sorted(kernels))
    assert found[0]["ScratchSize [bytes/lane]"] == 0, found[0]
