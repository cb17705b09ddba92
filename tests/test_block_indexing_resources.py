"""Build-time guard for the kernels that assemble an indexed plan on the device behind a stream's first decode
(hsrans_decode_device_indexing): k_index_count and k_index_fill (mt_ base plans), k_walk_index_count and k_walk_index_fill (block_ walk
plans), from the compiler's resource report as tests/test_kernel_resources.py reads it.  Each is in the code object once, and none spills
to scratch; their registers are reported as built (one workgroup and one wavefront per block of small kernels: nothing bounds their
occupancy)."""
import pytest

from test_kernel_resources import _report

KERNELS = ("k_index_count", "k_index_fill", "k_walk_index_count", "k_walk_index_fill")


@pytest.mark.parametrize("kernel", KERNELS)
def test_in_the_code_object_without_scratch(kernel):
    mangled = "%d%s" % (len(kernel), kernel)  # (the name with its length in front: k_index_count is also the end of k_walk_index_count)
    found = [r for name, r in _report("hsrans_kernels").items() if mangled in name]
    assert len(found) == 1, (kernel, len(found))
    r = found[0]
    print("%s: %d VGPRs, %d SGPRs, %d waves/SIMD, %d bytes of LDS" % (kernel, r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"], r["LDS Size [bytes/block]"]))
    assert r["ScratchSize [bytes/lane]"] == 0, (kernel, r)
