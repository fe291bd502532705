"""The input set of the portable Riesz functions (csrc/rz_trig.h), shared by tests/test_rz_trig.py (oracle and emulation build) and
tests/test_gpu_riesz_exact.py (the device): bit patterns, built with numpy.
  - every 64th pattern of all 2^32;
  - all patterns within 2^16 of +-0, +-0.5, +-1, the largest denormal and +-inf (the patterns behind inf are NaNs);
  - all patterns within 2^16 of every branch point of the implementation, read from the header's RZ_BP_* constants, and of the end
    of the range its accuracy statement covers (RZ_TRIG_ACCURATE), both signs;
  - for sin / cos: all patterns within 2^16 of the floats nearest k pi/4, k = 1 .. 32 (up to 8 pi), both signs."""
import functools
import os
import re

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "live-video-magnification_amd", "csrc", "rz_trig.h")
FNS = ("acos", "sin", "cos")
WINDOW = 1 << 16
BATCH = 1 << 24


def header_constants():
    """{name: float32 value} of the header's RZ_BP_* branch points and RZ_TRIG_ACCURATE"""
    text = open(HEADER, encoding="utf-8").read()
    found = dict(re.findall(r"#define (RZ_BP_\w+|RZ_TRIG_ACCURATE) ([0-9.eE+-]+)f\b", text))
    assert {"RZ_BP_ACOS_HALF", "RZ_BP_ACOS_ONE", "RZ_BP_TRIG_XMAX", "RZ_TRIG_ACCURATE"} <= set(found), sorted(found)
    # every RZ_BP_ name the code uses is one of the constants read above
    assert set(re.findall(r"\bRZ_BP_\w+", text)) == {k for k in found if k.startswith("RZ_BP_")}
    return {k: np.float32(v) for k, v in found.items()}


def _bits(values):
    return np.asarray(values, np.float32).view(np.uint32).astype(np.int64)


def _windows(centres):
    off = np.arange(-WINDOW, WINDOW + 1, dtype=np.int64)
    b = (np.unique(_bits(centres))[:, None] + off[None, :]).reshape(-1)
    return b[(b >= 0) & (b < (1 << 32))]


@functools.lru_cache(maxsize=None)
def inputs(fn):
    """float32 array (read-only) of the input set of `fn` ("acos" / "sin" / "cos"), no duplicates"""
    assert fn in FNS
    consts = header_constants()
    centres = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.inf, -np.inf]
    centres += [np.array([0x007FFFFF], np.uint32).view(np.float32)[0]]
    for v in consts.values():
        centres += [v, -v]
    if fn != "acos":
        k = np.arange(1, 33, dtype=np.float64)
        near = (k * (np.pi / 4)).astype(np.float32)
        centres += list(near) + list(-near)
    near = np.unique(_windows(centres))
    near = near[near % 64 != 0].astype(np.uint32)                  # (the multiples of 64 are in the stride already)
    x = np.concatenate([np.arange(1 << 26, dtype=np.uint32) * np.uint32(64), near]).view(np.float32)
    x.setflags(write=False)
    return x


def ordered(a):
    """float32 -> int64 that counts representable values along the number line (+-0 both 0); NaN patterns land beyond +-inf"""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    return np.abs(ordered(a) - ordered(b))


def same_bits(a, b):
    """bit equality, NaNs equal whatever their payload or sign: (all equal, number of differing values, index of the first)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    n = int(bad.sum())
    return n == 0, n, (int(np.flatnonzero(bad)[0]) if n else -1)


def reference(fn, x):
    """numpy.float32(numpy.arccos / sin / cos(float64(x)))"""
    f = {"acos": np.arccos, "sin": np.sin, "cos": np.cos}[fn]
    with np.errstate(invalid="ignore"):
        return f(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_values(po, fn):
    """po.trig_eval on inputs(fn), computed once per process (read-only)"""
    y = po.trig_eval(fn, inputs(fn))
    y.setflags(write=False)
    return y
