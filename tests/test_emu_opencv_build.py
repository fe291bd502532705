"""lvm_set_opencv_build on the CPU emulation build: the Riesz kernels under each build kind against the CPU oracle under the
matching switch (oracle/lvm_oracle.h LVMO_VAR_FILTER_UNFUSED / _FILTER_DFT / _MUL_F32), BIT FOR BIT in the exact flavour -- the
emulation build calls the host libm like the oracle does, so nothing but the kernels' own association is compared.

Every equality below is non-vacuous: oracle(kind) differs from oracle(0) on 9 .. 63 % of the float values of the first produced frame
of these clips (asserted per case), so a library that ignored the switch -- or an oracle whose switch were dead -- fails."""
import functools

import numpy as np
import pytest

from helpers import HostMem, c_params

HOST = HostMem()

UNFUSED, DFT, MUL_F32, ALL = 1, 2, 4, 7                       # LVM_CV_* (include/lvm_hip.h)
_ORACLE_BIT = {UNFUSED: "filter_unfused", DFT: "filter_dft", MUL_F32: "mul_f32"}
SIX_KINDS = [UNFUSED, DFT, MUL_F32, UNFUSED | MUL_F32, DFT | MUL_F32, DFT | UNFUSED]
# (67, 131, 2): odd sizes, two tile columns, scalar stores; (134, 78, 2): even but no multiple of 4, the compact collapse;
# (264, 150, 3): w % 4 == 0, two collapse levels
SHAPES = [(67, 131, 2), (134, 78, 2), (264, 150, 3)]
NFRAMES, CALLS = 7, (1, 2, 1, 3)

# every LVM_RZ_* forcing set of tests/test_gpu_exact.py::RZ_VARIANTS
RZ_VARIANTS = {
    "split_rows_10": {"LVM_RZ_SPLIT_ROWS_MIN": "1", "LVM_RZ_SPLIT_STRIP": "10"},
    "split_rows_54": {"LVM_RZ_SPLIT_ROWS_MIN": "1", "LVM_RZ_SPLIT_STRIP": "54"},
    "split_tiled": {"LVM_RZ_SPLIT_ROWS": "0", "LVM_RZ_SPLIT2_MIN": "1000000000"},
    "split2_phase4": {"LVM_RZ_SPLIT_ROWS": "0", "LVM_RZ_SPLIT2_MIN": "0", "LVM_RZ_PHASE4_MIN_FRAMES": "1"},
    "phase_narrow": {"LVM_RZ_PHASE4_MIN_FRAMES": "1000"},
    "blur4": {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_BLUR4": "1"},
    "blur_scalar": {"LVM_RZ_BLUR_STRIPS": "0", "LVM_RZ_BLUR4": "0"},
    "blur_strips_16": {"LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_BLUR_STRIP_ROWS": "16"},
    "blur_strips_64": {"LVM_RZ_BLUR_STRIPS_MIN": "0", "LVM_RZ_BLUR_STRIP_ROWS": "64"},
    "compact": {"LVM_RZ_COLLAPSE_STRIPS": "0", "LVM_RZ_COMPACT": "1"},
    "full_tile": {"LVM_RZ_COLLAPSE_STRIPS": "0", "LVM_RZ_COMPACT": "0"},
    "collapse_strips_10": {"LVM_RZ_COLLAPSE_STRIPS_MIN": "1", "LVM_RZ_COLLAPSE_STRIP": "10"},
    "collapse_strips_64": {"LVM_RZ_COLLAPSE_STRIPS_MIN": "1", "LVM_RZ_COLLAPSE_STRIP": "64"},
}
_RZ_ENV = sorted({k for v in RZ_VARIANTS.values() for k in v})


def oracle_mask(po, kind):
    return sum(po.VARIANTS[name] for bit, name in _ORACLE_BIT.items() if kind & bit)


@functools.lru_cache(maxsize=None)
def _clip_frames(lvm, idx, w, h, levels, n):
    ck, _ = lvm.synth.config(idx, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    frames = np.stack([clip.frame(t) for t in range(n)])
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _oracle_run(lvm, po, idx, w, h, levels, n, kinds):
    """[(produced, u8 frame, float frame or None)] of the clip with the oracle's variant switched to kinds[t] before frame t
    (computed once per case and shared; the arrays are read-only)"""
    frames = _clip_frames(lvm, idx, w, h, levels, n)
    _, pk = lvm.synth.config(idx, (w, h, levels))
    P = po.make_params(**pk)
    orc = po.Oracle()
    out = []
    try:
        for t in range(n):
            po.set_variant(oracle_mask(po, kinds[t]))
            u8, pr = orc.process(frames[t], P)
            u8 = np.array(u8)
            fl = orc.last_float().copy() if pr else None
            for a in (u8, fl):
                if a is not None:
                    a.setflags(write=False)
            out.append((pr, u8, fl))
    finally:
        po.set_variant(0)
        orc.close()
    return out


def _oracle(lvm, po, w, h, levels, kind, n=NFRAMES, idx=2):
    return _oracle_run(lvm, po, idx, w, h, levels, n, (kind,) * n)


def _assert_switch_is_alive(lvm, po, w, h, levels, kind):
    """oracle(kind) != oracle(0) on these very frames: matching oracle(kind) cannot be had by ignoring the switch"""
    r0, rk = _oracle(lvm, po, w, h, levels, 0), _oracle(lvm, po, w, h, levels, kind)
    assert [r[0] for r in r0] == [r[0] for r in rk]
    t = [r[0] for r in rk].index(True)
    share = float((r0[t][2] != rk[t][2]).mean())
    assert share > 0.05, "oracle(%d) and oracle(0) differ on %.1f %% of frame %d only" % (kind, 100 * share, t)


def _per_frame(lvm, emu, frames, pk, kinds, refs):
    """lvm_process, frame by frame; kinds[t] is set before frame t"""
    h, w = frames.shape[1:3]
    ctx = lvm.Context(0, 1, emu)
    ctx.keep_float(True)
    ctx.exact_lab(True)
    try:
        for t in range(len(frames)):
            ctx.set_opencv_build(kinds[t])
            assert ctx.opencv_build() == kinds[t]
            out, pg = ctx.process(frames[t], c_params(lvm, pk))
            pr, ref, fr = refs[t]
            assert pg == pr, "produced flag differs at frame %d: oracle %s, lib %s" % (t, pr, pg)
            if not pr:
                continue
            fg = ctx.read_float((h, w, 3))
            assert np.array_equal(fr, fg), "frame %d: %d float values differ from the oracle" % (t, int((fr != fg).sum()))
            assert np.array_equal(ref, out), "frame %d: %d bytes differ from the oracle" % (t, int((ref != out).sum()))
    finally:
        ctx.close()


def _batched(lvm, emu, frames, pk, kind, refs, calls=CALLS):
    """lvm_process_device_frames in calls of `calls` frames: every frame's bytes, and the float frame of each call's first frame"""
    n, h, w, _ = frames.shape
    assert sum(calls) == n
    fb = w * h * 3
    ctx = lvm.Context(0, 1, emu)
    ctx.keep_float(True)
    ctx.exact_lab(True)
    ctx.set_opencv_build(kind)
    try:
        d_in = HOST.upload(frames)
        d_out = HOST.zeros_like(d_in)
        t = 0
        for nf in calls:
            prod = ctx.process_device_frames(c_params(lvm, pk), nf, HOST.ptr(d_in, t), w, h, 3, w * 3, fb, fb, HOST.ptr(d_out, t), w * 3, fb, fb,
                                             HOST.stream())
            HOST.sync(ctx)
            assert prod == [refs[t + f][0] for f in range(nf)], (t, prod)
            if prod[0]:
                fg = ctx.read_float((h, w, 3))
                assert np.array_equal(refs[t][2], fg), "frame %d: %d float values differ from the oracle" % (t, int((refs[t][2] != fg).sum()))
            for f in range(nf):
                if prod[f]:
                    assert np.array_equal(refs[t + f][1], d_out[t + f]), "frame %d: %d bytes differ from the oracle" % (
                        t + f, int((refs[t + f][1] != d_out[t + f]).sum()))
            t += nf
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", SIX_KINDS)
@pytest.mark.parametrize("w,h,levels", SHAPES)
def test_riesz_build_kinds_emu_bit_exact(lvm, po, emu, w, h, levels, kind):
    frames = _clip_frames(lvm, 2, w, h, levels, NFRAMES)
    _, pk = lvm.synth.config(2, (w, h, levels))
    _assert_switch_is_alive(lvm, po, w, h, levels, kind)
    refs = _oracle(lvm, po, w, h, levels, kind)
    assert any(r[0] for r in refs)
    _per_frame(lvm, emu, frames, pk, (kind,) * NFRAMES, refs)
    _batched(lvm, emu, frames, pk, kind, refs)


@pytest.mark.parametrize("name", sorted(RZ_VARIANTS))
@pytest.mark.parametrize("kind", [UNFUSED | MUL_F32, DFT])
def test_one_arithmetic_per_kind_whatever_the_schedule(lvm, po, emu, kind, name, monkeypatch):
    """Every forcing set of the LVM_RZ_* switches still gives oracle(kind): the kernels that implement a kind are one arithmetic (the strip,
    vector and scalar forms of the phase and blur stages), and the 9 x 9 stages go to their kind-aware kernel whatever the switches say."""
    w, h, levels = 264, 150, 3
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in RZ_VARIANTS[name].items():
        monkeypatch.setenv(k, v)
    frames = _clip_frames(lvm, 2, w, h, levels, NFRAMES)
    _, pk = lvm.synth.config(2, (w, h, levels))
    _batched(lvm, emu, frames, pk, kind, _oracle(lvm, po, w, h, levels, kind))


def test_invalid_mask_changes_nothing(lvm, po, emu):
    w, h, levels = 67, 131, 2
    frames = _clip_frames(lvm, 2, w, h, levels, NFRAMES)
    _, pk = lvm.synth.config(2, (w, h, levels))
    refs = _oracle(lvm, po, w, h, levels, 0)
    ctx = lvm.Context(0, 1, emu)
    ctx.keep_float(True)
    ctx.exact_lab(True)
    try:
        assert ctx.opencv_build() == 0
        assert emu.lvm_set_opencv_build(ctx.h, 8) == -1                      # LVM_ERR_INVALID
        with pytest.raises(lvm.LvmError, match="lvm_set_opencv_build"):
            ctx.set_opencv_build(ALL | 16)
        assert ctx.opencv_build() == 0
        for t in range(3):
            out, pg = ctx.process(frames[t], c_params(lvm, pk))
            assert pg == refs[t][0]
            if pg:
                assert np.array_equal(refs[t][2], ctx.read_float((h, w, 3))) and np.array_equal(refs[t][1], out), t
        assert any(r[0] for r in refs[:3])
    finally:
        ctx.close()


@pytest.mark.parametrize("kinds", [(0, UNFUSED | MUL_F32), (DFT, UNFUSED), (ALL, 0)])
def test_switching_the_kind_mid_clip_keeps_the_state(lvm, po, emu, kinds):
    """The kind changes at frame 4; the temporal state is kept, as the oracle keeps it when its variant is switched at the same frame.
    lvm_reset keeps the kind (the context then follows an oracle that was reset under the same variant)."""
    w, h, levels = 134, 78, 2
    frames = _clip_frames(lvm, 2, w, h, levels, NFRAMES)
    _, pk = lvm.synth.config(2, (w, h, levels))
    sched = (kinds[0],) * 4 + (kinds[1],) * (NFRAMES - 4)
    refs = _oracle_run(lvm, po, 2, w, h, levels, NFRAMES, sched)
    same = _oracle(lvm, po, w, h, levels, kinds[0])
    assert any(r[0] and not np.array_equal(r[2], s[2]) for r, s in zip(refs[4:], same[4:])), "the switch at frame 4 changed nothing in the oracle"
    _per_frame(lvm, emu, frames, pk, sched, refs)
    # batched: calls of (1, 3) under the first kind, (2, 1) under the second
    fb = w * h * 3
    ctx = lvm.Context(0, 1, emu)
    ctx.exact_lab(True)
    try:
        d_in = HOST.upload(frames)
        d_out = HOST.zeros_like(d_in)
        t = 0
        for nf in (1, 3, 2, 1):
            ctx.set_opencv_build(sched[t])
            prod = ctx.process_device_frames(c_params(lvm, pk), nf, HOST.ptr(d_in, t), w, h, 3, w * 3, fb, fb, HOST.ptr(d_out, t), w * 3, fb, fb,
                                             HOST.stream())
            HOST.sync(ctx)
            for f in range(nf):
                assert prod[f] == refs[t + f][0]
                if prod[f]:
                    assert np.array_equal(refs[t + f][1], d_out[t + f]), "frame %d" % (t + f)
            t += nf
        ctx.reset()
        assert ctx.opencv_build() == kinds[1]
        again = _oracle(lvm, po, w, h, levels, kinds[1])
        for t in range(3):
            out, pg = ctx.process(frames[t], c_params(lvm, pk))
            assert pg == again[t][0]
            if pg:
                assert np.array_equal(again[t][1], out), "after reset, frame %d" % t
    finally:
        ctx.close()


@pytest.mark.parametrize("idx,nframes", [(0, 6), (3, 20)])
def test_laplace_and_color_ignore_the_kind(lvm, po, emu, idx, nframes):
    """LVM_CV_ALL on a Laplace and on a Color context: the mask-0 oracle, bit for bit (Color at 15 fps so that the window fills)."""
    w, h, levels = 96, 64, 3
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    if idx == 3:
        ck["fps"] = pk["framerate"] = 15.0
    clip = lvm.synth.Clip(**ck)
    P = po.make_params(**pk)
    orc = po.Oracle()
    ctx = lvm.Context(0, 1, emu)
    ctx.keep_float(True)
    ctx.exact_lab(True)
    ctx.set_opencv_build(ALL)
    produced = 0
    try:
        assert po.lib().lvmo_get_variant() == 0
        for t in range(nframes):
            f = clip.frame(t)
            ref, pr = orc.process(f, P)
            out, pg = ctx.process(f, c_params(lvm, pk))
            assert pr == pg, t
            if pr:
                produced += 1
                assert np.array_equal(orc.last_float(), ctx.read_float(ref.shape)) and np.array_equal(ref, out), "frame %d" % t
        assert produced >= 2
    finally:
        ctx.close()
        orc.close()


def kernel_selection(lvm, lib, mem):
    """lvm_profile_variants: under a kind the 9 x 9 stages run the kind-aware tiled kernels ("unfused" / "f64", level 0 collapsed by
    rz_collapse_l0 in front of the band-less last kernel), the phase and blur launches carry the kind; mask 0 reports none of it."""
    w, h, levels = 264, 150, 3
    frames = np.array(_clip_frames(lvm, 2, w, h, levels, NFRAMES))
    _, pk = lvm.synth.config(2, (w, h, levels))
    fb = w * h * 3
    seen = {}
    for kind in (0, UNFUSED | MUL_F32, DFT, ALL):
        ctx = lvm.Context(0, 1, lib)
        ctx.profile(True)
        ctx.set_opencv_build(kind)
        try:
            d_in = mem.upload(frames)
            d_out = mem.zeros_like(d_in)
            t = 0
            for nf in CALLS:
                ctx.process_device_frames(c_params(lvm, pk), nf, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3, fb, fb, mem.stream())
                t += nf
            mem.sync(ctx)
            variants = ctx.profile_variants()
            seen[kind] = {n: variants.get(n, set()) for n in ctx.profile_collect()}
        finally:
            ctx.close()
    kind_words = {"unfused", "f64", "mulf32", "unfused+mulf32"}
    assert not any(v & kind_words for v in seen[0].values()), seen[0]
    assert "rz_collapse_l0" not in seen[0]
    nine = ["rz_split_l0", "rz_split_l1", "rz_collapse_l1", "rz_collapse_l0"]
    s = seen[UNFUSED | MUL_F32]
    assert all(s[n] == {"unfused"} for n in nine), s
    assert s["rz_phase"] == {"unfused+mulf32"} and s["rz_blur_amp"] == {"unfused"} and s["rz_final"] == {"vec4"}, s
    s = seen[DFT]
    assert all(s[n] == {"f64"} for n in nine), s
    assert not (s["rz_phase"] | s["rz_blur_amp"]) and s["rz_final"] == {"vec4"}, s
    s = seen[ALL]
    assert all(s[n] == {"f64"} for n in nine), s
    assert s["rz_phase"] == {"unfused+mulf32"} and s["rz_blur_amp"] == {"unfused"}, s


def test_a_kind_runs_the_kernels_it_names_emu(lvm, emu):
    kernel_selection(lvm, emu, HOST)
