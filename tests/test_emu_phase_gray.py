"""lvm_set_phase_on_gray on the CPU emulation build: LVM_MODE_PHASE on 1-channel frames against the CPU oracle fed the expanded frames,
followed by BGR2GRAY (tests/phase_gray.py), BIT FOR BIT in the exact and the analytic flavour -- float frame, bytes and produced flags.

Every equality with the reference is non-vacuous: the reference differs from the input on more than half of the pixels (asserted per
case; 99 % on these clips), so a library that handed the gray frames back fails.  The one exception is levels = 1: a pyramid without
band levels magnifies nothing, there the float frame (Lab -> BGR of the per-value table) and the produced flags carry the test."""
import numpy as np
import pytest

import phase_gray as pg
from helpers import HostMem, c_params
from test_emu_opencv_build import RZ_VARIANTS, _RZ_ENV

HOST = HostMem()
UNFUSED, DFT, MUL_F32 = 1, 2, 4
INVALID = -1                                                       # LVM_ERR_INVALID


def _per_frame(lvm, ctx, frames, pk, refs):
    """lvm_process frame by frame: flags, float frame (three channels) and bytes"""
    h, w = frames.shape[1:]
    for t in range(len(frames)):
        out, p = ctx.process(frames[t], c_params(lvm, pk))
        pr, gray, fl = refs[t]
        assert p == pr, "produced flag differs at frame %d: reference %s, lib %s" % (t, pr, p)
        if not pr:
            assert np.array_equal(out, frames[t])
            continue
        fg = ctx.read_float((h, w, 3))
        assert np.array_equal(fl, fg), "frame %d: %d float values differ from the reference" % (t, int((fl != fg).sum()))
        assert np.array_equal(gray, out), "frame %d: %d bytes differ from the reference" % (t, int((gray != out).sum()))


def _batched(lvm, emu, streams, pk, refs, flavour="exact", kind=0, mem=HOST):
    """lvm_process_device_frames in calls of (1, 2, 1, 3): every stream's bytes, stream 0's float frame at the head of each call"""
    ctx = pg.context(lvm, emu, len(streams), flavour, kind=kind)

    def check_float(t, fg):
        assert np.array_equal(refs[0][t][2], fg), "frame %d: %d float values differ from the reference" % (t, int((refs[0][t][2] != fg).sum()))
    try:
        prod, outs = pg.run_frames(lvm, ctx, mem, streams, pk, check_float=check_float)
        for s, r in enumerate(refs):
            pg.assert_equals_reference(prod, outs[:, s], r, "stream %d" % s)
    finally:
        ctx.close()


@pytest.mark.parametrize("flavour", ["exact", "analytic"])
@pytest.mark.parametrize("w,h,levels", pg.SHAPES + [(96, 64, 1)])
def test_gray_phase_is_the_oracle_on_the_expanded_frames(lvm, po, emu, w, h, levels, flavour):
    analytic = flavour == "analytic"
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0, analytic)
    if levels > 1:
        pg.assert_not_vacuous(frames, refs)
    else:
        assert any(r[0] for r in refs)
    ctx = pg.context(lvm, emu, 1, flavour)
    try:
        _per_frame(lvm, ctx, frames, pk, refs)
    finally:
        ctx.close()
    _batched(lvm, emu, [frames], pk, [refs], flavour)
    other = pg.gray_clip(lvm, po, w, h, levels, seed=1235)
    _batched(lvm, emu, [frames, other], pk, [refs, pg.clip_reference(lvm, po, w, h, levels, 0, analytic, seed=1235)], flavour)


@pytest.mark.parametrize("kind", [UNFUSED, DFT | MUL_F32])
@pytest.mark.parametrize("w,h,levels", pg.SHAPES)
def test_gray_phase_under_the_build_kinds(lvm, po, emu, w, h, levels, kind):
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, kind)
    plain = pg.clip_reference(lvm, po, w, h, levels, 0)
    pg.assert_not_vacuous(frames, refs)
    assert any(r[0] and not np.array_equal(r[2], q[2]) for r, q in zip(refs, plain)), "the kind changes nothing in the oracle"
    ctx = pg.context(lvm, emu, 1, "exact", kind=kind)
    try:
        _per_frame(lvm, ctx, frames, pk, refs)
    finally:
        ctx.close()
    _batched(lvm, emu, [frames], pk, [refs], kind=kind)


@pytest.mark.parametrize("name", sorted(RZ_VARIANTS))
def test_gray_phase_whatever_the_schedule(lvm, po, emu, name, monkeypatch):
    """every forcing set of the LVM_RZ_* switches: the same bytes and floats (the strip output forced onto 264 x 150 among them)"""
    w, h, levels = 264, 150, 3
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in RZ_VARIANTS[name].items():
        monkeypatch.setenv(k, v)
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0)
    pg.assert_not_vacuous(frames, refs)
    _batched(lvm, emu, [frames], pk, [refs])
    if name.startswith("collapse_strips"):
        assert _variants(lvm, emu, frames, pk)["rz_final"] == {"gray-strips"}


def _variants(lvm, lib, frames, pk, flavour="exact", keep_float=False):
    ctx = pg.context(lvm, lib, 1, flavour, keep_float=keep_float)
    ctx.profile(True)
    try:
        pg.run_frames(lvm, ctx, HOST, [frames], pk)
        v = ctx.profile_variants()
        return {n: v.get(n, set()) for n in ctx.profile_collect()}
    finally:
        ctx.close()


# ---- all 256 gray values ---------------------------------------------------------------------------------------------------------
def _ramp_clip():
    """256 x 16, two levels (256 x 8 holds one level only, lvm_max_levels, and a pyramid without bands magnifies nothing): a noise frame,
    then the frame whose columns are the values 0 .. 255, then another noise frame -- the ramp and the noise are the second and third
    frame, so both are produced"""
    rng = np.random.default_rng(20241)
    ramp = np.tile(np.arange(256, dtype=np.uint8), (16, 1))
    return np.stack([rng.integers(0, 256, ramp.shape, dtype=np.uint8), ramp, rng.integers(0, 256, ramp.shape, dtype=np.uint8)])


def _ramp_not_vacuous(frames, outs):
    """the noise frame changes on more than half of its pixels; the ramp -- no texture along y, one gradient along x: little to magnify --
    changes somewhere"""
    assert float((outs[2] != frames[2]).mean()) > 0.5 and (outs[1] != frames[1]).any()


@pytest.mark.parametrize("flavour", ["exact", "analytic"])
def test_every_gray_value_goes_through_the_table(lvm, po, emu, flavour):
    """the synthetic clip only holds the values 8 .. 183: here every entry of the per-value table is read, on both ends of the chain"""
    frames = _ramp_clip()
    h, w = frames.shape[1:]
    assert sorted(np.unique(frames[1])) == list(range(256)) and emu.lvm_max_levels(w, h) >= 2
    pk = dict(pg.params(lvm, w, h, 2), levels=2)
    refs = pg.reference(po, frames, pk, 0, flavour == "analytic")
    assert [r[0] for r in refs] == [False, True, True]
    _ramp_not_vacuous(frames, [r[1] for r in refs])
    ctx = pg.context(lvm, emu, 1, flavour)
    try:
        _per_frame(lvm, ctx, frames, pk, refs)
    finally:
        ctx.close()


@pytest.mark.parametrize("strips", [False, True])
def test_every_gray_value_default_flavour_equals_the_bgr_path(lvm, po, emu, strips, monkeypatch):
    """the shipped configuration (default flavour, no float frame: the u8 step table in the strip kernel) has no bit-exact oracle; its
    definition is the library's own BGR path on the expanded frames, byte for byte"""
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    if strips:
        monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS_MIN", "1")
    frames = _ramp_clip()
    h, w = frames.shape[1:]
    pk = dict(pg.params(lvm, w, h, 2), levels=2)
    a = pg.context(lvm, emu, 1, "default", keep_float=False)
    b = pg.context(lvm, emu, 1, "default", keep_float=False, on=False)
    try:
        a.profile(True)
        outs = []
        for t in range(len(frames)):
            out, p = a.process(frames[t], c_params(lvm, pk))
            ref, q = b.process(pg.expand(frames[t]), c_params(lvm, pk))
            assert p == q == (t > 0)
            if p:
                assert np.array_equal(out, po.bgr2gray_u8(ref)), "frame %d: %d bytes differ from the BGR path" % (t, int((out != po.bgr2gray_u8(ref)).sum()))
            outs.append(out)
        _ramp_not_vacuous(frames, outs)
        assert a.profile_variants()["rz_final"] == ({"gray-strips"} if strips else {"gray4"})
    finally:
        a.close(); b.close()


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
# (input offset, output offset, row stride - w): the dword forms need w % 4 == 0 and dword-aligned pointers, row and stream strides
LAYOUTS = {
    "packed": (0, 0, 0, "gray4", "gray4"),
    "padded_rows": (0, 0, 8, "gray4", "gray4"),
    "odd_input_pointer": (1, 0, 8, "gray", "gray"),
    "odd_output_pointer": (0, 3, 8, "gray4", "gray"),
    "odd_row_stride": (0, 0, 5, "gray", "gray"),
}


@pytest.mark.parametrize("strips", [False, True])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_byte_and_dword_kernels_agree(lvm, po, emu, name, strips, monkeypatch):
    """the same clip through every layout: the reference's bytes, the kernel the launch code must pick (lvm_profile_variants), and
    not a byte outside the w x h rectangles of the 0xAB canvas"""
    w, h, levels = 264, 150, 3
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    if strips:
        monkeypatch.setenv("LVM_RZ_COLLAPSE_STRIPS_MIN", "1")
    off_in, off_out, pad, front, back = LAYOUTS[name]
    if strips and back == "gray4":
        back = "gray-strips"
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0)
    row = w + pad
    fs = h * row
    total = 16 + pg.NFRAMES * fs + 64
    buf_in = np.full(total, 0xAB, np.uint8)
    idx = (np.arange(pg.NFRAMES)[:, None, None] * fs + np.arange(h)[None, :, None] * row + np.arange(w)[None, None, :])
    buf_in[off_in + idx] = frames
    buf_out = np.full(total, 0xAB, np.uint8)
    assert buf_in.ctypes.data % 16 == 0 and buf_out.ctypes.data % 16 == 0
    ctx = pg.context(lvm, emu, 1, "exact", keep_float=False)
    ctx.profile(True)
    try:
        prod, t = [], 0
        for nf in pg.CALLS:
            prod += ctx.process_device_frames(c_params(lvm, pk), nf, buf_in.ctypes.data + off_in + t * fs, w, h, 1, row, fs, fs,
                                              buf_out.ctypes.data + off_out + t * fs, row, fs, fs, None)
            t += nf
        ctx.synchronize()
        v = ctx.profile_variants()
    finally:
        ctx.close()
    pg.assert_equals_reference(prod, buf_out[off_out + idx], refs, name)
    untouched = np.ones(total, bool)
    untouched[(off_out + idx[np.asarray(prod, bool)]).reshape(-1)] = False
    bad = np.flatnonzero(untouched & (buf_out != 0xAB))
    assert bad.size == 0, "%d bytes outside the output rectangles were written, first at offset %d" % (bad.size, int(bad[0]))
    assert v["lab_lut"] == {front} and v["rz_final"] == {back}, v


def test_analytic_flavour_reports_under_rz_lab(lvm, po, emu):
    w, h, levels = 264, 150, 3
    v = _variants(lvm, emu, pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels), "analytic")
    assert v["rz_lab"] == {"gray4"} and "lab_lut" not in v and v["rz_final"] == {"gray4"}, v


# ---- option semantics --------------------------------------------------------------------------------------------------------------
def test_off_by_default_and_on_produces(lvm, po, emu):
    """Off (the default): gray Phase frames produce nothing, as in the reference (MagnifyCore.hpp:212).  On: the same calls produce --
    the test that fails without the feature."""
    w, h, levels = 67, 131, 2
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0)
    ctx = pg.context(lvm, emu, 1, "exact", on=False)
    try:
        assert ctx.phase_on_gray() is False
        for t in range(4):
            out, p = ctx.process(frames[t], c_params(lvm, pk))
            assert not p and np.array_equal(out, frames[t])
        ctx.set_phase_on_gray(True)
        assert ctx.phase_on_gray() is True
        _per_frame(lvm, ctx, frames, pk, refs)
        assert sum(r[0] for r in refs) >= 5
    finally:
        ctx.close()


def test_invalid_value_changes_nothing(lvm, po, emu):
    ctx = pg.context(lvm, emu, 1, "exact", on=False)
    try:
        assert emu.lvm_set_phase_on_gray(ctx.h, 2) == INVALID and emu.lvm_set_phase_on_gray(ctx.h, -1) == INVALID
        with pytest.raises(lvm.LvmError, match="lvm_set_phase_on_gray"):
            ctx.set_phase_on_gray(2)
        assert ctx.phase_on_gray() is False
        ctx.set_phase_on_gray(True)
        assert emu.lvm_set_phase_on_gray(ctx.h, 2) == INVALID
        assert ctx.phase_on_gray() is True
    finally:
        ctx.close()


def test_switching_mid_clip_restarts_and_reset_keeps_the_option(lvm, po, emu):
    w, h, levels = 134, 78, 2
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0)
    tail = pg.reference(po, frames[3:], pk)                        # the clip from frame 3 on: a first frame, then produced frames
    assert not tail[0][0] and all(r[0] for r in tail[1:])
    ctx = pg.context(lvm, emu, 1, "exact")
    try:
        _per_frame(lvm, ctx, frames[:3], pk, refs[:3])
        ctx.set_phase_on_gray(True)                                # the value it has: nothing happens
        out, p = ctx.process(frames[3], c_params(lvm, pk))
        assert p and np.array_equal(out, refs[3][1])
        ctx.set_phase_on_gray(False)                               # a structural change: the state is dropped ...
        out, p = ctx.process(frames[3], c_params(lvm, pk))
        assert not p and np.array_equal(out, frames[3])
        ctx.set_phase_on_gray(True)                                # ... and the next frame is a first frame
        _per_frame(lvm, ctx, frames[3:], pk, tail)
        ctx.reset()
        assert ctx.phase_on_gray() is True
        _per_frame(lvm, ctx, frames, pk, refs)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["bgr_phase", "gray_laplace", "gray_color"])
def test_other_clips_ignore_the_option(lvm, po, emu, case):
    """BGR Phase, gray Laplace and gray Color clips: identical bytes and flags with the option on and off"""
    idx, n = {"bgr_phase": (2, 6), "gray_laplace": (0, 6), "gray_color": (3, 20)}[case]
    ck, pk = lvm.synth.config(idx, (96, 64, 3))
    if idx == 3:
        ck["fps"] = pk["framerate"] = 15.0                         # (the window fills inside the clip)
    clip = lvm.synth.Clip(**ck)
    frames = [clip.frame(t) if case == "bgr_phase" else po.bgr2gray_u8(clip.frame(t)) for t in range(n)]
    res = []
    for on in (False, True):
        ctx = pg.context(lvm, emu, 1, "default", keep_float=False, on=on)
        try:
            res.append([ctx.process(f, c_params(lvm, pk)) for f in frames])
        finally:
            ctx.close()
    assert sum(p for _, p in res[0]) >= 2
    for t, ((a, pa), (b, pb)) in enumerate(zip(*res)):
        assert pa == pb and np.array_equal(a, b), t


def test_switching_under_another_key_only_stores(lvm, po, emu):
    """a BGR Phase clip keeps its temporal state across a change of the option"""
    w, h, levels = 96, 64, 2
    ck, pk = lvm.synth.config(2, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    ctx = pg.context(lvm, emu, 1, "default", keep_float=False, on=False)
    try:
        assert not ctx.process(clip.frame(0), c_params(lvm, pk))[1]
        assert ctx.process(clip.frame(1), c_params(lvm, pk))[1]
        ctx.set_phase_on_gray(True)
        assert ctx.process(clip.frame(2), c_params(lvm, pk))[1]     # (a dropped state would make this a first frame)
    finally:
        ctx.close()


def test_cutoff_change_follows_the_oracle(lvm, po, emu):
    w, h, levels = 134, 78, 2
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    pk2 = dict(pk, coLow=pk["coLow"] * 1.5, coHigh=pk["coHigh"] * 1.25)
    pks = [pk] * 4 + [pk2] * (pg.NFRAMES - 4)
    refs = pg.reference(po, frames, pks)
    same = pg.clip_reference(lvm, po, w, h, levels, 0)
    assert any(r[0] and not np.array_equal(r[1], s[1]) for r, s in zip(refs[4:], same[4:])), "the cutoff change at frame 4 changed nothing in the oracle"
    ctx = pg.context(lvm, emu, 1, "exact")
    try:
        for t in range(pg.NFRAMES):
            out, p = ctx.process(frames[t], c_params(lvm, pks[t]))
            assert p == refs[t][0], t
            if p:
                assert np.array_equal(refs[t][2], ctx.read_float((h, w, 3))) and np.array_equal(refs[t][1], out), "frame %d" % t
    finally:
        ctx.close()


def test_set_lab_lut_and_flavour_changes_reach_the_table(lvm, po, emu):
    """the per-value table follows lvm_debug_lab_analytic and lvm_set_lab_lut on a LIVE gray state (same structural key, the state is kept)"""
    w, h, levels = 67, 131, 2
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    ctx = pg.context(lvm, emu, 1, "exact")
    bgr = pg.context(lvm, emu, 1, "exact", on=False)
    try:
        table = ctx.lab_lut().copy()
        for t in range(6):
            if t == 2:
                ctx.lab_analytic(True); bgr.lab_analytic(True)
            if t == 4:
                ctx.lab_analytic(False); bgr.lab_analytic(False)
                table[0::3] = np.minimum(table[0::3] + 37, 16384)   # another forward table: every L entry moved
                ctx.synchronize(); bgr.synchronize()
                ctx.set_lab_lut(table); bgr.set_lab_lut(table)
            out, p = ctx.process(frames[t], c_params(lvm, pk))
            ref, q = bgr.process(pg.expand(frames[t]), c_params(lvm, pk))
            assert p == q == (t > 0)
            if p:
                assert np.array_equal(ctx.read_float((h, w, 3)), bgr.read_float((h, w, 3))), t
                assert np.array_equal(out, po.bgr2gray_u8(ref)), t
    finally:
        ctx.close(); bgr.close()


# ---- the chain and the export ------------------------------------------------------------------------------------------------------
def test_chain_and_export_with_the_grayscale_toggle(lvm, po, emu):
    """lvm_chain_process with grayscale = 1 on a BGR source and lvm_export_frames with LVM_SPLIT_LEFT_RIGHT: the processed pane is the
    reference of the preprocessed gray frames"""
    w, h, levels = 128, 96, 2
    ck, pk = lvm.synth.config(2, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    src = [clip.frame(t) for t in range(6)]
    cpre = lvm.LvmPreprocessParams(2, 0, 0.0, 0.0, 1.0, 1.0, 1)
    opre, otap = po.PreParams(2, 0, 0.0, 0.0, 1.0, 1.0, 1), po.PreParams(2, 0, 0.0, 0.0, 1.0, 1.0, 0)
    small = np.stack([po.preprocess(f, opre) for f in src])
    assert small.ndim == 3 and small.shape[1:] == (h // 2, w // 2)
    refs = pg.reference(po, small, pk)
    pg.assert_not_vacuous(small, refs)
    ctx = pg.context(lvm, emu, 1, "exact", keep_float=False)
    try:
        for t in range(6):
            out, p = ctx.chain_process(src[t], cpre, c_params(lvm, pk))
            assert p == refs[t][0], t
            assert np.array_equal(out, refs[t][1] if p else small[t]), "chain, frame %d" % t
        ctx.reset()
        t = 0
        for nb in (1, 2, 3):
            canvases, prod = ctx.export_frames(src[t:t + nb], cpre, c_params(lvm, pk), 1)        # LVM_SPLIT_LEFT_RIGHT
            for k in range(nb):
                pr, gray, _ = refs[t + k]
                assert prod[k] == pr, t + k
                want = po.compose(1, po.preprocess(src[t + k], otap), gray if pr else small[t + k])
                assert want is not None and np.array_equal(canvases[k], want), "export, frame %d" % (t + k)
            t += nb
    finally:
        ctx.close()
