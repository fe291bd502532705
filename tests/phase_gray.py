"""Shared pieces of the gray Phase tests (tests/test_emu_phase_gray.py, tests/test_gpu_phase_gray.py; test infrastructure).

The feature (lvm_set_phase_on_gray, include/lvm_hip.h): a Phase context fed the gray frames g_t gives, frame by frame,
    produced_t, out_t == produced'_t, BGR2GRAY(Riesz(expand(g_t)))
The clips are lvm.synth config 2 converted with po.bgr2gray_u8; the reference is the oracle fed expand(g), followed by
po.bgr2gray_u8; float frames are the oracle's last_float() of the expanded frame (three channels)."""
import functools

import numpy as np

from helpers import c_params

NFRAMES, CALLS = 7, (1, 2, 1, 3)
# (67, 131, 2): odd sizes, byte I/O; (134, 78, 2): even, no multiple of 4, compact collapse; (264, 150, 3): w % 4 == 0, dword I/O, two collapse levels
SHAPES = [(67, 131, 2), (134, 78, 2), (264, 150, 3)]
_ORACLE_BIT = {1: "filter_unfused", 2: "filter_dft", 4: "mul_f32"}       # LVM_CV_* -> the oracle's switch of the same name


def expand(g):
    """the BGR frame(s) with b = g = r = g"""
    return np.repeat(np.asarray(g)[..., None], 3, axis=-1)


@functools.lru_cache(maxsize=None)
def gray_clip(lvm, po, w, h, levels, n=NFRAMES, seed=None):
    """[n][h][w] uint8, read-only: config 2, gray-converted"""
    ck, _ = lvm.synth.config(2, (w, h, levels))
    clip = lvm.synth.Clip(**ck) if seed is None else lvm.synth.Clip(seed=seed, **ck)
    frames = np.stack([po.bgr2gray_u8(clip.frame(t)) for t in range(n)])
    frames.setflags(write=False)
    return frames


def params(lvm, w, h, levels):
    return lvm.synth.config(2, (w, h, levels))[1]


def reference(po, frames, pks, kind=0, analytic=False, portable_trig=False):
    """[(produced, gray u8 frame, BGR float frame or None)] of the gray frames: the oracle on expand(g) with the parameters pks[t]
    (a dict: the same for every frame), under the build kind `kind` and the forward Lab flavour, then BGR2GRAY.  portable_trig: the
    oracle's LVMO_VAR_PORTABLE_TRIG besides (csrc/rz_trig.h: what the library computes under LVM_RZ_PORTABLE_TRIG).  The oracle's
    variant mask is put back to what it was."""
    if isinstance(pks, dict):
        pks = [pks] * len(frames)
    orc = po.Oracle()
    out = []
    po.lib().lvmo_set_lab_lut(0 if analytic else 1)
    before = int(po.lib().lvmo_get_variant())
    po.set_variant(sum(po.VARIANTS[name] for bit, name in _ORACLE_BIT.items() if kind & bit) | (po.VARIANTS["portable_trig"] if portable_trig else 0))
    try:
        for g, pk in zip(frames, pks):
            u8, pr = orc.process(expand(g), po.make_params(**pk))
            gray = np.array(po.bgr2gray_u8(u8))
            fl = orc.last_float().copy() if pr else None
            for a in (gray, fl):
                if a is not None:
                    a.setflags(write=False)
            out.append((bool(pr), gray, fl))
    finally:
        po.set_variant(before)
        po.lib().lvmo_set_lab_lut(1)
        orc.close()
    return out


@functools.lru_cache(maxsize=None)
def clip_reference(lvm, po, w, h, levels, kind=0, analytic=False, n=NFRAMES, seed=None, portable_trig=False):
    """reference() of gray_clip(), computed once per case and shared (read-only arrays)"""
    return tuple(reference(po, gray_clip(lvm, po, w, h, levels, n, seed), params(lvm, w, h, levels), kind, analytic, portable_trig))


def assert_not_vacuous(frames, refs):
    """the reference differs from the input on more than half of the pixels of every produced frame: equality with it cannot be had
    by handing the input back"""
    assert any(r[0] for r in refs)
    for t, (pr, gray, _) in enumerate(refs):
        if pr:
            share = float((gray != frames[t]).mean())
            assert share > 0.5, "frame %d: the reference differs from the input on %.1f %% of the pixels only" % (t, 100 * share)


def context(lvm, lib, n_streams=1, flavour="exact", keep_float=True, kind=0, on=True):
    """flavour: "exact" (lvm_debug_exact_lab), "analytic" (lvm_debug_lab_analytic) or "default" (the shipped configuration)"""
    ctx = lvm.Context(0, n_streams, lib)
    ctx.keep_float(keep_float)
    ctx.exact_lab(flavour == "exact")
    ctx.lab_analytic(flavour == "analytic")
    ctx.set_opencv_build(kind)
    if on:
        ctx.set_phase_on_gray(True)
    return ctx


def run_frames(lvm, ctx, mem, streams, pk, calls=CALLS, check_float=None):
    """lvm_process_device_frames on gray frames, `streams` = one [n][h][w] clip per stream of the context, packed [frame][stream]; returns
    (produced flags [n], outputs [n][stream][h][w]).  check_float(t, float frame of stream 0): called for the first frame of every call
    that produced (what lvm_debug_keep_float keeps of a batch)."""
    fin = np.stack(streams, axis=1)                                   # [n][stream][h][w]
    n, S, h, w = fin.shape
    fb = w * h
    d_in = mem.upload(fin)
    d_out = mem.zeros_like(d_in)
    prod, t = [], 0
    for nf in calls:
        p = ctx.process_device_frames(c_params(lvm, pk), nf, mem.ptr(d_in, t), w, h, 1, w, fb, fb * S, mem.ptr(d_out, t), w, fb, fb * S, mem.stream())
        mem.sync(ctx)
        if check_float is not None and p[0]:
            check_float(t, ctx.read_float((h, w, 3)))
        prod += p
        t += nf
    assert t == n
    return prod, np.array(mem.download(d_out))


def assert_equals_reference(prod, outs, refs, what=""):
    """flags frame by frame, bytes of every produced frame"""
    assert list(prod) == [r[0] for r in refs], (what, prod)
    for t, (pr, gray, _) in enumerate(refs):
        if pr:
            assert np.array_equal(gray, outs[t]), "%s frame %d: %d bytes differ from the reference" % (what, t, int((gray != outs[t]).sum()))
