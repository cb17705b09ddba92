"""The library's HSRANS_* switches are read in one place, read_tuning() (csrc/hsrans_tuning.cpp), and taken by an object when it is
made: a getenv anywhere else would be read at a launch again, or from threads that share nothing else.  Two names stay where they are
used, since neither has a context: HSRANS_DEVICE (drop-in entries) and HSRANS_CPU_WIDE_MODE (host decoder)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")
ELSEWHERE = {"hsrans_dropin.cpp": {"HSRANS_DEVICE"}, "hsrans_cpu.cpp": {"HSRANS_CPU_WIDE_MODE"}}


def _sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path.endswith((".cpp", ".h", ".hip")):
            yield os.path.basename(path), open(path).read()


def test_getenv_only_in_read_tuning():
    stray = []
    for name, text in _sources():
        if name == "hsrans_tuning.cpp":
            continue
        for m in re.finditer(r"\bgetenv\s*\(([^)]*)\)", text):
            arg = m.group(1).strip().strip('"')
            if arg not in ELSEWHERE.get(name, set()):
                stray.append(f"{name}:{text.count(chr(10), 0, m.start()) + 1}: getenv({m.group(1)})")
    assert not stray, "environment read outside read_tuning(): " + "; ".join(stray)


def test_every_switch_documented():
    text = open(os.path.join(CSRC, "hsrans_tuning.cpp")).read()
    names = set(re.findall(r'"(HSRANS_[A-Z0-9_]+)"', text))
    assert len(names) >= 30
    readme = open(os.path.join(ROOT, "README.md")).read()
    documented = set(re.findall(r"`(HSRANS_[A-Z0-9_]+)[=`]", readme))  # (each name in full, in backticks, with or without its values)
    missing = sorted(names - documented)
    assert not missing, f"switches read by read_tuning() but not in README's environment table: {missing}"
