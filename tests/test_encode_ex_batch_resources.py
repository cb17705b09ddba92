"""Build-time guard for hsrans_encode_device_ex_batch: the compiler's resource report (csrc/build/hsrans_encode.remarks) lists its four
kernels — the chain for both state counts — none spills to scratch, and a batched kernel needs no more registers and LDS than the single
call's kernel whose code it runs."""
import pytest

import kernel_remarks

NS = "_ZN6hsrans12_GLOBAL__N_1"


@pytest.fixture(scope="module")
def kernels():
    return kernel_remarks.read("hsrans_encode")


def _one(kernels, mangled_prefix):
    return kernel_remarks.one(kernels, NS + mangled_prefix)


# (mangled: length-prefixed name, then for the chain the state count as a template argument)
NEW = {"summaries": "22k_unit_summaries_batchE", "costs": "18k_unit_costs_batchE", "chain64": "20k_encode_chain_batchILj64EE", "chain32": "20k_encode_chain_batchILj32EE",
       "gather": "20k_gather_chain_batchE"}
OLD = {"summaries": "16k_unit_summariesE", "costs": "12k_unit_costsE", "chain64": "14k_encode_chainILj64EE", "chain32": "14k_encode_chainILj32EE", "gather": "14k_gather_chainE"}


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_the_batch_kernels_exist_and_do_not_spill(kernels, kernel):
    assert _one(kernels, NEW[kernel])["ScratchSize [bytes/lane]"] == 0


@pytest.mark.parametrize("kernel", ("chain64", "chain32", "summaries"))
def test_a_batch_kernel_needs_no_more_than_the_single_calls(kernels, kernel):
    new, old = _one(kernels, NEW[kernel]), _one(kernels, OLD[kernel])
    assert new["VGPRs"] <= old["VGPRs"], (new, old)
    assert new["LDS Size [bytes/block]"] <= old["LDS Size [bytes/block]"], (new, old)
