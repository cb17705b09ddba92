"""Build-time guard for the kernels of hsrans_decode_device_indexing_batch, from the compiler's resource report and the built object's ISA as
tests/test_kernel_resources.py reads them: k_index_pass_batch in its three table layouts and the batch forms of the four assembly kernels are
in the code object exactly as often as they are instantiated, none spills to scratch, the four single-stream assembly kernels are still
there under their names, and the recording pass's decode loops do not begin with a wait on the vector-memory counter (the rule that file
applies to k_decode<MODE, false>, whose device functions the pass calls)."""
import os
import re

import pytest

from test_kernel_resources import LLVM, _disassemble, _report

ASSEMBLY = ("k_index_count", "k_index_fill", "k_walk_index_count", "k_walk_index_fill")


def _found(kernel):
    mangled = "%d%s" % (len(kernel), kernel)  # (the name with its length in front: k_index_count is also the end of k_walk_index_count)
    return [(name, r) for name, r in _report("hsrans_kernels").items() if mangled in name]


def test_the_recording_pass_is_there_in_three_layouts_without_scratch():
    found = _found("k_index_pass_batch")
    assert sorted(re.search(r"k_index_pass_batchILi(\d)E", name).group(1) for name, _ in found) == ["0", "1", "2"], [name for name, _ in found]
    for name, r in found:
        print("%s: %d VGPRs, %d SGPRs, %d waves/SIMD" % (name, r["VGPRs"], r["TotalSGPRs"], r["Occupancy [waves/SIMD]"]))
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


@pytest.mark.parametrize("kernel", [k + "_batch" for k in ASSEMBLY])
def test_the_batch_assembly_kernels_are_there_once_without_scratch(kernel):
    found = _found(kernel)
    assert len(found) == 1, (kernel, [name for name, _ in found])
    assert found[0][1]["ScratchSize [bytes/lane]"] == 0, found[0]


@pytest.mark.parametrize("kernel", ASSEMBLY)
def test_the_single_stream_assembly_kernels_keep_their_names(kernel):
    found = _found(kernel)
    assert len(found) == 1, (kernel, [name for name, _ in found])
    assert found[0][1]["ScratchSize [bytes/lane]"] == 0, found[0]


@pytest.mark.skipif(not os.path.exists(LLVM + "/llvm-objdump"), reason="needs the ROCm LLVM tools")
def test_the_pass_loops_do_not_drain_the_memory_queue(tmp_path):
    text = _disassemble(tmp_path)
    funcs = {}  # name -> list of (address, mnemonic + operands, branch target or None)
    cur, base = None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            base, cur = int(m.group(1), 16), funcs.setdefault(m.group(2), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s+// ([0-9A-F]+): ", line)
        if not m or cur is None:
            continue
        target = None
        t = re.search(r"<\S+\+0x([0-9a-f]+)>\s*$", line)
        if t and m.group(1).startswith(("s_branch", "s_cbranch")):
            target = base + int(t.group(1), 16)
        cur.append((int(m.group(2), 16), m.group(1), target))
    per_kernel = {}
    for name, ins in funcs.items():
        if "k_index_pass_batchILi" not in name:
            continue
        addr_index = {a: i for i, (a, _, _) in enumerate(ins)}
        loops = [(addr_index[t], i) for i, (a, _, t) in enumerate(ins) if t is not None and t < a and t in addr_index]
        groups = lambda lo, hi: sum(1 for _, s, _ in ins[lo:hi + 1] if s.startswith("v_mbcnt_hi"))
        per_kernel[name] = 0
        for lo, hi in loops:
            # the innermost loops that hold four decode groups or more
            if groups(lo, hi) < 4 or any((l2, h2) != (lo, hi) and l2 >= lo and h2 <= hi and groups(l2, h2) >= 4 for l2, h2 in loops):
                continue
            head = [s for _, s, _ in ins[lo:lo + 8]]
            assert not any(s.startswith("s_waitcnt") and "vmcnt" in s for s in head), (name, hex(ins[lo][0]), head)
            per_kernel[name] += 1
    assert len(per_kernel) == 3 and all(n >= 1 for n in per_kernel.values()), per_kernel
