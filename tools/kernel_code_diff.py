#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of an object file, kernel by kernel:  kernel_code_diff.py [--show NAME-SUBSTRING] OLD.o NEW.o

Extracts the gfx950 code object from each (as tests/test_kernel_resources.py::_disassemble does), disassembles it and, per
kernel, strips addresses, encodings and branch-target offsets.  Prints each kernel's two instruction counts and whether the two
texts are identical.  Used to show that a refactor of the device code left the kernels as they were.

A kernel is a symbol with a kernel descriptor (NAME.kd in the symbol table).  Any other label inside .text — the named labels of
inline assembly land in the symbol table too — belongs to the kernel it lies in and starts nothing.

--show NAME-SUBSTRING also prints a unified diff of the two instruction lists of every kernel whose (demangled) name contains it."""
import argparse
import difflib
import re
import shutil
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    """name -> list of instructions (mnemonic + operands; a branch's target offset is replaced by '<>')"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = tmp + "/fat.bin", tmp + "/k.co"
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--unbundle", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        symbols = subprocess.check_output([LLVM + "/llvm-objdump", "-t", co], text=True)
        text = subprocess.check_output([LLVM + "/llvm-objdump", "-d", co], text=True)
    with_descriptor = {line.split()[-1][:-3] for line in symbols.splitlines() if line.endswith(".kd")}
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            if m.group(1) in with_descriptor:
                cur = out.setdefault(m.group(1), [])
            continue  # (any other label: part of the kernel it lies in)
        m = re.match(r"^\s+(\S.*?)\s+// [0-9A-F]+: ", line)
        if m and cur is not None:
            ins = m.group(1)
            if ins.startswith(("s_branch", "s_cbranch", "s_call", "s_getpc", "s_setpc")):
                ins = ins.split()[0] + " <>"
            cur.append(ins)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--show", metavar="NAME-SUBSTRING", help="print a unified diff of the matching kernels' instruction lists")
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    names = sorted(set(old) | set(new))
    filt = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    shown_as = subprocess.check_output([filt] + names, text=True).splitlines() if filt and names else names
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
    if args.show is not None:
        for name, shown in zip(names, shown_as):
            if args.show in shown or args.show in name:
                diff = list(difflib.unified_diff(old.get(name, []), new.get(name, []), "OLD " + shown, "NEW " + shown, lineterm=""))
                print("\n".join(diff) if diff else "(no difference: %s)" % shown)


if __name__ == "__main__":
    main()
