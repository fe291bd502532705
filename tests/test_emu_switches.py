"""Every launch switch and every run-time kernel instantiation, on the CPU emulation build (the cases: tests/parity_matrix.py,
SWITCH_CASES; the gfx950 twin: tests/test_gpu_switches.py).  All three modes equal the oracle bit for bit here, and every case asserts
the report name and variant of the kernel it is there for.  Besides: values the switches' validators refuse (emulation only -- such a
value must never reach a kernel, so no GPU test sets one) and LVM_ZERO_COPY=0 in a child process."""
import os
import subprocess
import sys

import pytest

import parity_matrix as M
from helpers import HostMem

HOST = HostMem()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Not on the emulation: ten levels (3072 x 2564; k_lap_collapse<8>), four times the pixels of the nine-level case (1536 x 1284, <7>), which
# takes the emulation 15 to 45 s depending on what else runs: under the minute it was given, so it runs here.  k_lap_collapse<9> and
# <10> need frames of at least 5121 x 5121 and 10241 x 10241: untested on every build (tests/parity_matrix.py, DEEP).
GPU_ONLY = {"deep10"}
EMU_CASES = [k for k in M.SWITCH_CASES if k not in GPU_ONLY]
REQUIRED = M.REQUIRED - {("lap_collapse", "n8")}


@pytest.mark.parametrize("key", EMU_CASES)
def test_switch_case_emu(lvm, po, emu, key):
    M.switch_case(lvm, po, emu, HOST, "emu", key)


def test_big_up_geometry_is_the_threshold():
    """LVM_UP_DEPTH_BIG is read from 1024 tiled workgroups at a level: the case's geometry has them at level 1, one stream fewer has not"""
    w, h, _, ns = M.BIG_UP
    assert M.tiled_up_blocks(w, h, ns) >= 1024 > M.tiled_up_blocks(w, h, ns - 1), (M.up_tile(), M.tiled_up_blocks(w, h, ns))


def test_every_runtime_instantiation_is_reached(lvm, po, emu):
    seen = M.ledger(lvm, po, emu, HOST, "emu", [k for k in M.LEDGER_KEYS if k not in GPU_ONLY])
    assert REQUIRED <= seen, sorted(REQUIRED - seen)


# ---- refused values: the default's bytes, names and variants -----------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(M.REFUSED_CASES))
def test_refused_value_keeps_the_default(lvm, po, emu, key):
    """bit-equal to the oracle, and launch for launch what the same case launches with the refused switch unset"""
    prof = M.switch_case(lvm, po, emu, HOST, "emu", key)
    env = dict(M.REFUSED_CASES[key][3])
    del env[M.REFUSED_SWITCH[key]]
    _, base = M.switch_run(lvm, emu, HOST, key, env=env)
    assert prof == [r[4] for r in base], (key, prof, [r[4] for r in base])


# ---- LVM_ZERO_COPY=0: read once per process, so a child process ---------------------------------------------------------------------
ZERO_COPY_CHILD = """
import ctypes, importlib, os, sys
sys.path[:0] = [{root!r}, {tests!r}]
assert os.environ["LVM_ZERO_COPY"] == "0"
lvm = importlib.import_module("live-video-magnification_amd")
import test_preprocess as T
lib = lvm.bind(ctypes.CDLL({lib!r})) if {lib!r} else lvm.load()
T._check_pinned_equals_pageable(lvm, lib, {sizes!r})
print("zero-copy off: pinned frames equal pageable frames")
"""
EMU_SIZES = [(0, (64, 48, 3), False, 0), (2, (64, 48, 3), False, 20), (3, (64, 48, 2), False, 4), (0, (64, 48, 3), True, 8)]


def zero_copy_off_child(lib_path, sizes, timeout):
    """tests/test_preprocess.py's pinned-equals-pageable check in a fresh process with LVM_ZERO_COPY=0: staged copies for pinned frames"""
    code = ZERO_COPY_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=lib_path, sizes=sizes)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LVM_ZERO_COPY="0"), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "zero-copy off" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_zero_copy_off_emu(emu):
    zero_copy_off_child(emu._name, EMU_SIZES, 300)
