"""csrc/rz_trig.h -- rz_acosf / rz_sinf / rz_cosf, the one implementation of the three transcendental functions that the oracle
(LVMO_VAR_PORTABLE_TRIG) and the exact-flavour Riesz kernels (LVM_RZ_PORTABLE_TRIG) share.  On the input set of tests/rz_trig_set.py:

  accuracy   po.trig_eval against numpy.float32(numpy.arccos / sin / cos(float64(x))): at most 1 ulp everywhere in [-1, 1] (acos) and for
             |x| <= 100 pi (sin / cos).  One ulp is no measurement: the functions evaluate in float64 (error below 2^-40 relative) and
             round once, which lands on the correctly rounded float or on its neighbour.  The share of results that are not the
             reference's is printed (-s) and recorded in DESIGN.md 5, not asserted.  The kernels only ask for [0, pi].
  beyond     every other finite argument of sin / cos: finite and |y| <= 1; acos beyond +-1: the end values; inf / NaN: NaN.
  emulation  lvm_debug_trig_eval of the CPU emulation build (the kernel the gfx950 build runs, compiled by the host compiler) equals
             po.trig_eval bit for bit -- NaNs compare equal whatever their payload.  tests/test_gpu_riesz_exact.py asks the same of the device."""
import numpy as np
import pytest

import rz_trig_set as T
from helpers import HostMem

HOST = HostMem()
F32 = np.float32
PI_F = F32(np.pi)


def _domain(fn, x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= (F32(1.0) if fn == "acos" else T.header_constants()["RZ_TRIG_ACCURATE"])


def test_the_accurate_range_is_100_pi():
    c = T.header_constants()
    assert c["RZ_TRIG_ACCURATE"] == F32(100 * np.pi) and c["RZ_BP_TRIG_XMAX"] > c["RZ_TRIG_ACCURATE"]
    assert c["RZ_BP_ACOS_HALF"] == F32(0.5) and c["RZ_BP_ACOS_ONE"] == F32(1.0)


@pytest.mark.parametrize("fn", T.FNS)
def test_one_ulp_of_the_float64_reference(po, fn):
    x, y = T.inputs(fn), T.oracle_values(po, fn)
    assert x.size > (1 << 26) and np.unique(x.view(np.uint32)).size == x.size
    m = _domain(fn, x)
    ref = T.reference(fn, x[m])
    d = T.ulp_distance(y[m], ref)
    off = float((d != 0).mean())
    kernel = m & (x >= 0) & (x <= PI_F) if fn != "acos" else m
    dk = T.ulp_distance(y[kernel], T.reference(fn, x[kernel]))
    print("rz_%sf: %d arguments in the stated range, worst %d ulp, %.3e of them not the float64 reference rounded once; the kernels' range: %d arguments, worst %d ulp, %.3e"
          % (fn, int(m.sum()), int(d.max()), off, int(kernel.sum()), int(dk.max()), float((dk != 0).mean())))
    worst = int(np.argmax(d))
    assert d.max() <= 1, "rz_%sf(%r) = %r, reference %r: %d ulp" % (fn, x[m][worst], y[m][worst], ref[worst], int(d.max()))


@pytest.mark.parametrize("fn", T.FNS)
def test_every_float_gives_a_defined_result(po, fn):
    x, y = T.inputs(fn), T.oracle_values(po, fn)
    nan, inf = np.isnan(x), np.isinf(x)
    assert nan.any() and inf.any()
    assert np.isnan(y[nan]).all(), "NaN in, a number out"
    fin = ~nan & ~inf
    assert not np.isnan(y[fin]).any() and np.isfinite(y[fin]).all()
    if fn == "acos":
        assert (y[x >= 1] == 0).all() and (y[x <= -1] == PI_F).all()                  # the end values, inf included
        assert (y[fin] >= 0).all() and (y[fin] <= PI_F).all()
    else:
        assert np.isnan(y[inf]).all()
        assert (np.abs(y[fin]) <= 1).all()
        big = np.abs(x) > T.header_constants()["RZ_BP_TRIG_XMAX"]
        assert (big & fin).any() and (y[big & fin] == (0 if fn == "sin" else 1)).all()
    again = po.trig_eval(fn, x[:: 1 << 10])
    assert T.same_bits(again, y[:: 1 << 10])[0]                                      # deterministic


def test_known_answers(po):
    acos = lambda *v: po.trig_eval("acos", np.array(v, F32))                         # noqa: E731
    sin = lambda *v: po.trig_eval("sin", np.array(v, F32))                           # noqa: E731
    cos = lambda *v: po.trig_eval("cos", np.array(v, F32))                           # noqa: E731
    assert np.array_equal(acos(1, -1, 0, -0.0), np.array([0, np.pi, np.pi / 2, np.pi / 2], F32))
    assert np.array_equal(acos(0.5, -0.5), np.array([np.pi / 3, 2 * np.pi / 3], F32))
    assert np.array_equal(acos(1.5, -1.5, 3e38, -3e38, np.inf, -np.inf), np.array([0, np.pi] * 3, F32))
    assert np.isnan(acos(np.nan)).all() and np.isnan(sin(np.nan, np.inf, -np.inf)).all() and np.isnan(cos(np.nan, np.inf, -np.inf)).all()
    s0 = sin(0.0, -0.0)
    assert np.array_equal(s0, np.zeros(2, F32)) and np.signbit(s0[1]) and not np.signbit(s0[0])
    assert np.array_equal(cos(0.0, -0.0), np.ones(2, F32))
    h, p = F32(np.pi / 2), PI_F                                                        # the floats nearest pi/2 and pi: the exact values of
    assert np.array_equal(sin(h, p), np.array([1.0, np.sin(np.float64(p))], F32))      # sin / cos there are 1 - 1e-15, -8.7e-8, -4.4e-8, -1 + 4e-15
    assert np.array_equal(cos(h, p), np.array([np.cos(np.float64(h)), -1.0], F32))
    assert sin(p)[0] == F32(-8.742278e-08) and cos(h)[0] == F32(-4.371139e-08)
    assert np.array_equal(sin(-h, -p), -sin(h, p)) and np.array_equal(cos(-h, -p), cos(h, p))


@pytest.mark.parametrize("fn", T.FNS)
def test_emulation_build_equals_the_oracle(lvm, po, emu, fn):
    x, want = T.inputs(fn), T.oracle_values(po, fn)
    got = np.empty_like(want)
    ctx = lvm.Context(0, 1, emu)
    try:
        for i in range(0, x.size, T.BATCH):
            d_x = HOST.upload(x[i:i + T.BATCH])
            d_y = HOST.zeros_like(d_x)
            ctx.trig_eval(po.TRIG_FNS[fn], d_x.ctypes.data, d_y.ctypes.data, d_x.size, HOST.stream())
            HOST.sync(ctx)
            got[i:i + T.BATCH] = HOST.download(d_y)
    finally:
        ctx.close()
    ok, n, first = T.same_bits(got, want)
    assert ok, "rz_%sf: %d of %d values differ, first at x = %r (bits %#010x): emulation %r, oracle %r" % (
        fn, n, x.size, x[first], int(x.view(np.uint32)[first]), got[first], want[first])


def test_the_debug_entry_refuses_what_it_cannot_run(lvm, emu):
    ctx = lvm.Context(0, 1, emu)
    try:
        a = np.zeros(4, F32)
        for fn, px, py in ((3, a.ctypes.data, a.ctypes.data), (-1, a.ctypes.data, a.ctypes.data), (0, None, a.ctypes.data), (0, a.ctypes.data, None)):
            with pytest.raises(lvm.LvmError):
                ctx.trig_eval(fn, px, py, 4)
        ctx.trig_eval(0, None, None, 0)                                               # nothing to do is no error
    finally:
        ctx.close()
