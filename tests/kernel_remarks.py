"""The compiler's per-kernel resource report (-Rpass-analysis=kernel-resource-usage), which csrc/Makefile keeps next to each device
object as csrc/build/<unit>.remarks: the one reader the *_resources.py tests share."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
BUILD = os.path.join(CSRC, "build")


def read(unit):
    """{function: {field: int}} of csrc/build/<unit>.remarks; the library is built first where the report is missing."""
    path = os.path.join(BUILD, unit + ".remarks")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    kernels, cur = {}, None
    for line in open(path).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def one(kernels, prefix):
    """The report of the one function whose mangled name starts with `prefix`."""
    found = [r for name, r in kernels.items() if name.startswith(prefix)]
    assert len(found) == 1, (prefix, sorted(kernels))
    return found[0]
