#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of an object file, kernel by kernel:  kernel_code_diff.py OLD.o NEW.o

Extracts the gfx950 code object from each (as tests/test_kernel_resources.py::_disassemble does), disassembles it and, per
kernel, strips addresses, encodings and branch-target offsets.  Prints each kernel's two instruction counts and whether the two
texts are identical.  Used to show that a refactor of the device code left the kernels as they were."""
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    """name -> list of instructions (mnemonic + operands; a branch's target offset is replaced by '<>')"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = tmp + "/fat.bin", tmp + "/k.co"
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--unbundle", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        text = subprocess.check_output([LLVM + "/llvm-objdump", "-d", co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+(\S.*?)\s+// [0-9A-F]+: ", line)
        if m and cur is not None:
            ins = m.group(1)
            if ins.startswith(("s_branch", "s_cbranch", "s_call", "s_getpc", "s_setpc")):
                ins = ins.split()[0] + " <>"
            cur.append(ins)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(old) | set(new))
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    shown_as = subprocess.check_output([filt] + names, text=True).splitlines() if filt else names
    same = 0
    for name, shown in zip(names, shown_as):
        a, b = old.get(name), new.get(name)
        if a is None or b is None:
            verdict = "only in " + ("NEW" if a is None else "OLD")
        else:
            verdict = "identical" if a == b else "DIFFERENT"
            same += a == b
        print("%6s %6s  %-9s  %s" % ("-" if a is None else len(a), "-" if b is None else len(b), verdict, shown))
    print("%d kernels, %d identical" % (len(names), same))


if __name__ == "__main__":
    main()
