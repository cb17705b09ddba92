"""Build-time guard for the pack kernel: the compiler's resource report (csrc/build/hsrans_planes_pack.remarks) lists exactly k_pack, and
it neither spills to scratch nor uses LDS (a lane holds HSRANS_PACK_CHUNK / 4096 units of 16 bytes in registers between its loads and its
stores)."""
import kernel_remarks

NAME = "_ZN6hsrans12_GLOBAL__N_16k_packE"  # (mangled: length-prefixed name, then the arguments)


def test_the_report_lists_exactly_k_pack_without_scratch_or_lds():
    kernels = kernel_remarks.read("hsrans_planes_pack")
    assert len(kernels) == 1 and next(iter(kernels)).startswith(NAME), sorted(kernels)
    report = next(iter(kernels.values()))
    assert report["ScratchSize [bytes/lane]"] == 0 and report["LDS Size [bytes/block]"] == 0, report
