"""Build-time guard for the batch range-merge kernel: the compiler's resource report (csrc/build/hsrans_planes_gather_batch.remarks) lists
exactly the one kernel — k_planes_merge_ranges_batch, which serves 2-, 4- and 8-byte members in one launch — and it neither spills to
scratch nor uses LDS (like the single call's kernels, it holds a block's elements and planes in registers)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "hypersonic_rans_amd", "csrc", "build")
NS = "_ZN6hsrans12_GLOBAL__N_1"
KERNEL = "27k_planes_merge_ranges_batchE"  # (mangled: length-prefixed name, then the argument types)


@pytest.fixture(scope="module")
def kernels():
    path = os.path.join(BUILD, "hsrans_planes_gather_batch.remarks")
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


def test_the_report_lists_exactly_the_one_kernel(kernels):
    assert len(kernels) == 1, sorted(kernels)
    assert next(iter(kernels)).startswith(NS + KERNEL), sorted(kernels)


def test_the_kernel_neither_spills_nor_uses_lds(kernels):
    (found,) = kernels.values()
    assert found["ScratchSize [bytes/lane]"] == 0, found
    assert found["LDS Size [bytes/block]"] == 0, found
