"""lvm_set_opencv_build on the MI355X: the Riesz mode against the CPU oracle under the matching build switch
(oracle/lvm_oracle.h LVMO_VAR_FILTER_UNFUSED / _FILTER_DFT / _MUL_F32).

Without the setter the library computes ONE association, and against an oracle that stands for an SSE2-dispatch or an ARM / macOS
OpenCV it misses the parity bar: oracle(0) <-> oracle(unfused) and oracle(0) <-> oracle(dft) are 1.2e-4 / 99.74 % and 1.2e-4 / 99.72 %
on the clip below, the bar is 1e-4 / 99.9 %.  With the kind set the bar is met (test_build_kind_meets_the_parity_bar).

What separates library(kind) from oracle(kind) on the GPU is the device library's acosf / sinf / cosf against glibc's (and, in the
default flavour, the reciprocal / hardware-transcendental forms of the well-conditioned steps): bit equality is the CPU emulation
build's business (tests/test_emu_opencv_build.py)."""
import functools

import numpy as np
import pytest

from helpers import TorchMem, c_params
from test_emu_opencv_build import CALLS, DFT, MUL_F32, NFRAMES, RZ_VARIANTS, SHAPES, UNFUSED, _RZ_ENV, _clip_frames, _oracle, _oracle_run, kernel_selection

pytestmark = pytest.mark.gpu

FLOAT_TOL, U8_MAX, U8_FRAC = 1e-4, 1, 0.999            # the parity bar
BIG = (320, 180, 5)                                      # the clip of test_variant_envelope_gpu: BASELINE config 2, 64 frames
BIG_N = 64
BUILD_KINDS = [UNFUSED, DFT, DFT | MUL_F32]
KIND_NAMES = {0: "default", UNFUSED: "unfused", DFT: "dft", MUL_F32: "mul_f32", DFT | MUL_F32: "dft|mul_f32", UNFUSED | MUL_F32: "unfused|mul_f32"}


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


def _big_oracle(lvm, po, kind):
    w, h, levels = BIG
    return _oracle_run(lvm, po, 2, w, h, levels, BIG_N, (kind,) * BIG_N)


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_runs():
    yield
    _oracle_run.cache_clear()
    _big_library_mask0_exact.cache_clear()


def _big_library(lvm, hip, kind, exact, keep_float):
    """[(float frame or None, u8 frame) or None per frame] of the 64-frame clip through lvm_process with the kind set"""
    w, h, levels = BIG
    frames = _clip_frames(lvm, 2, w, h, levels, BIG_N)
    _, pk = lvm.synth.config(2, BIG)
    ctx = lvm.Context(0, 1, hip)
    ctx.keep_float(keep_float)
    ctx.exact_lab(exact)
    ctx.set_opencv_build(kind)
    got = []
    try:
        for f in frames:
            out, pg = ctx.process(f, c_params(lvm, pk))
            got.append(((ctx.read_float(f.shape).copy() if keep_float else None), out.copy()) if pg else None)
    finally:
        ctx.close()
    return got


@functools.lru_cache(maxsize=None)
def _big_library_mask0_exact(lvm, hip):
    return _big_library(lvm, hip, 0, True, True)


def _float_distance(got, refs):
    """worst frame of max|d| / max|ref| over the produced frames"""
    rel = 0.0
    for g, (pr, _, fr) in zip(got, refs):
        assert pr == (g is not None)
        if pr:
            rel = max(rel, float(np.abs(fr - g[0]).max() / np.abs(fr).max()))
    return rel


@pytest.mark.parametrize("kind", BUILD_KINDS)
def test_build_kind_meets_the_parity_bar(lvm, po, hip, kind):
    """The shipped configuration (default flavour, no keep_float) with the kind set, against oracle(kind): float rel <= 1e-4 (from a
    second, float-keeping context), <= 1 LSB, >= 99.9 % identical bytes on EVERY produced frame.  Against oracle(0) -- all the library
    could compute before lvm_set_opencv_build -- these oracles are 1.2e-4 / 99.72-99.74 % away."""
    refs = _big_oracle(lvm, po, kind)
    ship = _big_library(lvm, hip, kind, False, False)
    keep = _big_library(lvm, hip, kind, False, True)
    worst = [0.0, 0, 1.0]
    assert any(r[0] for r in refs)
    for t, (s_, k_, (pr, ref, fr)) in enumerate(zip(ship, keep, refs)):
        assert pr == (s_ is not None) == (k_ is not None), t
        if not pr:
            continue
        rel = float(np.abs(fr - k_[0]).max() / np.abs(fr).max())
        du = np.abs(ref.astype(np.int32) - s_[1].astype(np.int32))
        worst = [max(worst[0], rel), max(worst[1], int(du.max())), min(worst[2], float((du == 0).mean()))]
    print("HIP[%-11s] vs oracle[%-11s] cfg2 %s x %d frames: float %.2e  u8 max %d  identical %.5f" % (
        KIND_NAMES[kind], KIND_NAMES[kind], BIG, BIG_N, worst[0], worst[1], worst[2]))
    assert worst[0] <= FLOAT_TOL and worst[1] <= U8_MAX and worst[2] >= U8_FRAC, worst


@pytest.mark.parametrize("kind", [UNFUSED, DFT, MUL_F32])
def test_each_kind_is_closest_to_its_own_oracle(lvm, po, hip, kind):
    """Exact flavour, worst-frame float distance over the 64 frames: library(kind) is closer to oracle(kind) than to oracle(0), and
    library(0) closer to oracle(0) than to oracle(kind).  oracle(0) <-> oracle(kind) is 1.2e-4 / 1.2e-4 / 1.2e-5; the device library's
    acosf / sinf / cosf against glibc's is what the library adds (<= 5.6e-7 over 7-frame clips)."""
    o0, ok = _big_oracle(lvm, po, 0), _big_oracle(lvm, po, kind)
    l0, lk = _big_library_mask0_exact(lvm, hip), _big_library(lvm, hip, kind, True, True)
    d = {"lib(k)-orc(k)": _float_distance(lk, ok), "lib(k)-orc(0)": _float_distance(lk, o0),
         "lib(0)-orc(0)": _float_distance(l0, o0), "lib(0)-orc(k)": _float_distance(l0, ok)}
    print("exact flavour, k = %-8s" % KIND_NAMES[kind], "  ".join("%s %.2e" % kv for kv in d.items()))
    assert d["lib(k)-orc(k)"] < d["lib(k)-orc(0)"], d
    assert d["lib(0)-orc(0)"] < d["lib(0)-orc(k)"], d


def _run(lvm, hip, dev, monkeypatch, frames, pk, kind, env, keep_float, exact, calls=CALLS):
    """(produced flags, u8 frames, float frame of each call's first frame) through lvm_process_device_frames (calls=None:
    lvm_process_device, frame by frame)"""
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, h, w, _ = frames.shape
    fb = w * h * 3
    ctx = lvm.Context(0, 1, hip)
    ctx.keep_float(keep_float)
    ctx.exact_lab(exact)
    ctx.set_opencv_build(kind)
    try:
        d_in = dev.upload(frames)
        d_out = dev.zeros_like(d_in)
        prod, floats, t = [], [], 0
        if calls is None:
            for t in range(n):
                prod.append(ctx.process_device(c_params(lvm, pk), dev.ptr(d_in, t), w, h, 3, w * 3, fb, dev.ptr(d_out, t), w * 3, fb, dev.stream()))
            dev.sync(ctx)
            return prod, dev.download(d_out), floats
        for nf in calls:
            prod += ctx.process_device_frames(c_params(lvm, pk), nf, dev.ptr(d_in, t), w, h, 3, w * 3, fb, fb, dev.ptr(d_out, t), w * 3, fb, fb,
                                              dev.stream())
            t += nf
            dev.sync(ctx)
            floats.append(ctx.read_float((h, w, 3)).copy() if keep_float and prod[t - nf] else None)
        return prod, dev.download(d_out), floats
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", [UNFUSED | MUL_F32, DFT])
@pytest.mark.parametrize("w,h,levels", SHAPES)
def test_small_shapes_vector_and_byte_kernels(lvm, po, hip, dev, w, h, levels, kind, monkeypatch):
    """Odd sizes (byte I/O, scalar stores), even sizes that are no multiple of 4 (the compact collapse), w % 4 == 0 with two collapse
    levels, in calls of (1, 2, 1, 3) frames:
      - exact flavour: oracle(kind)'s produced flags, bytes within 1 LSB / >= 99.9 % of oracle(kind);
      - default flavour: per-frame lvm_process_device calls give the bytes of the batched calls;
      - default flavour: every LVM_RZ_* forcing set gives the bytes and the float frames of the unforced run on this GPU -- one
        arithmetic per kind, whichever kernels the switches pick."""
    frames = np.array(_clip_frames(lvm, 2, w, h, levels, NFRAMES))
    _, pk = lvm.synth.config(2, (w, h, levels))
    refs = _oracle(lvm, po, w, h, levels, kind)
    prod, u8, _ = _run(lvm, hip, dev, monkeypatch, frames, pk, kind, {}, False, True)
    assert prod == [r[0] for r in refs] and any(prod)
    for t in range(NFRAMES):
        if prod[t]:
            du = np.abs(refs[t][1].astype(np.int32) - u8[t].astype(np.int32))
            assert du.max() <= U8_MAX and (du == 0).mean() >= U8_FRAC, (t, int(du.max()), float((du == 0).mean()))
    base = {kf: _run(lvm, hip, dev, monkeypatch, frames, pk, kind, {}, kf, False) for kf in (True, False)}
    assert base[True][0] == base[False][0] == prod
    pprod, pu8, _ = _run(lvm, hip, dev, monkeypatch, frames, pk, kind, {}, False, False, calls=None)
    assert pprod == prod
    for t in range(NFRAMES):
        if prod[t]:
            assert np.array_equal(pu8[t], base[False][1][t]), "frame %d: %d bytes of the per-frame calls differ from the batched calls" % (
                t, int((pu8[t] != base[False][1][t]).sum()))
    for name, env in sorted(RZ_VARIANTS.items()):
        for kf in (True, False):
            vprod, vu8, vfl = _run(lvm, hip, dev, monkeypatch, frames, pk, kind, env, kf, False)
            assert vprod == prod, (name, kf)
            for t in range(NFRAMES):
                if prod[t]:
                    assert np.array_equal(vu8[t], base[kf][1][t]), "%s keep_float=%s frame %d: %d bytes differ from the unforced run" % (
                        name, kf, t, int((vu8[t] != base[kf][1][t]).sum()))
            for a, b in zip(vfl, base[kf][2]):
                assert (a is None) == (b is None)
                if a is not None:
                    assert np.array_equal(a, b), "%s: %d float values differ from the unforced run" % (name, int((a != b).sum()))


def test_a_kind_runs_the_kernels_it_names(lvm, hip, dev):
    kernel_selection(lvm, hip, dev)
