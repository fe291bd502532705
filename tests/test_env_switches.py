"""Every LVM_* switch a test sets is read by the library: a renamed or removed switch would otherwise turn a variant test into a
second run of the default kernels without anyone noticing."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(pattern):
    return {p: open(p, encoding="utf-8", errors="replace").read() for p in glob.glob(os.path.join(ROOT, pattern)) if os.path.isfile(p)}


def test_every_switch_the_tests_set_is_read_by_the_library():
    csrc = "\n".join(_read("live-video-magnification_amd/csrc/*").values())
    read = {n for line in csrc.splitlines() if "env_switch(" in line for n in re.findall(r'"(LVM_[A-Z0-9_]+)"', line)}
    assert len(read) > 30, sorted(read)
    tests = _read("tests/*.py")
    used = {}
    for path, text in tests.items():
        for name in re.findall(r'setenv\(\s*"(LVM_[A-Z0-9_]+)"', text):
            used.setdefault(name, set()).add(os.path.basename(path))
        # switch tables handed to monkeypatch.setenv in a loop: {"LVM_...": "value"} entries
        for name in re.findall(r'"(LVM_[A-Z0-9_]+)"\s*:\s*"', text):
            used.setdefault(name, set()).add(os.path.basename(path))
    used.pop("LVM_EMU_LIB", None)          # the emulation fixture's library path (tests/conftest.py), not a library switch
    assert "LVM_RZ_SPLIT_STRIP" in used and "LVM_COL_OUT_ROWS" in used, sorted(used)
    missing = {n: sorted(f) for n, f in used.items() if n not in read}
    assert not missing, "switches set by tests but read by no env_switch in csrc/: %s" % missing
