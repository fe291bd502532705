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


# Switches the library reads and no test sets: {name: reason}, two at the most.
UNTESTED = {}


def _switches_tests_set():
    """{switch: files}: monkeypatch.setenv("LVM_...", ...) calls, and "LVM_...": / dict(..., LVM_...=value) entries of the switch tables that tests hand
    to setenv or os.environ in a loop"""
    used = {}
    for path, text in _read("tests/*.py").items():
        if os.path.basename(path) == os.path.basename(__file__):
            continue
        for pat in (r'setenv\(\s*"(LVM_[A-Z0-9_]+)"', r'"(LVM_[A-Z0-9_]+)"\s*:', r'[(,]\s*(LVM_[A-Z0-9_]+)=(?:"|str\(|[a-z_]+[,)])'):
            for name in re.findall(pat, text):
                used.setdefault(name, set()).add(os.path.basename(path))
    return used


def test_every_switch_the_library_reads_is_set_by_a_test():
    """the converse: a switch no test sets selects a kernel, a loop bound or a copy path that ships untested"""
    read = set()
    for text in _read("live-video-magnification_amd/csrc/*").values():
        for line in text.splitlines():
            if "env_switch(" in line and "inline bool env_switch" not in line:
                names = re.findall(r'"(LVM_[A-Z0-9_]+)"', line)
                assert names, "an env_switch call whose switch name this test cannot read: %s" % line.strip()
                read |= set(names)
    assert len(read) > 50, sorted(read)
    assert len(UNTESTED) <= 2 and all(isinstance(r, str) and len(r) > 20 for r in UNTESTED.values()), UNTESTED
    assert set(UNTESTED) <= read, "UNTESTED names switches the library does not read: %s" % sorted(set(UNTESTED) - read)
    used = _switches_tests_set()
    stale = sorted(n for n in UNTESTED if n in used)
    assert not stale, "listed in UNTESTED but set by a test: %s" % stale
    missing = sorted(read - set(used) - set(UNTESTED))
    assert not missing, "switches read by csrc/ that no test sets: %s" % missing
