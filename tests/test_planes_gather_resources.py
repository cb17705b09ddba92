"""Build-time guard for the range-merge kernels: the compiler's resource report (csrc/build/hsrans_planes_gather.remarks) lists exactly the
three kernels — k_planes_merge_ranges for 2-, 4- and 8-byte elements — and none of them spills to scratch or uses LDS (like the two
whole-frame kernels, they hold a block's elements and planes in registers)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "hypersonic_rans_amd", "csrc", "build")
NS = "_ZN6hsrans12_GLOBAL__N_1"
# (mangled: length-prefixed name, then the element size as a template argument)
KERNELS = {f"W{W}": f"21k_planes_merge_rangesILj{W}EE" for W in (2, 4, 8)}


@pytest.fixture(scope="module")
def kernels():
    path = os.path.join(BUILD, "hsrans_planes_gather.remarks")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "hypersonic_rans_amd", "csrc")])
    out, cur = {}, None
    for line in open(path).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


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
