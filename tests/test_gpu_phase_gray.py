"""lvm_set_phase_on_gray on the MI355X (tests/phase_gray.py has the definition and the reference).

Two questions, small shapes, a few seconds each:
  - the library against itself in the shipped configuration (default flavour, no float frame): a context with the option on, fed the
    gray clip, against a second context fed the expanded clip whose bytes go through BGR2GRAY on the host.  IDENTICAL bytes, no
    tolerance: both sides run the same arithmetic on the same device -- per frame and in batches, one and two streams, the strip
    output forced;
  - against the CPU oracle at the bars of the BGR Riesz tests (tests/helpers.py run_pair): float 1e-4 relative, <= 1 LSB, >= 99.9 %
    identical bytes, equal produced flags.  What separates the two is the device library's acosf / sinf / cosf against glibc's and
    the default flavour's reciprocal forms; the gray weighting cannot widen a <= 1 LSB difference (its weights add up to 1).
Bit equality with the oracle is the emulation build's business (tests/test_emu_phase_gray.py)."""
import numpy as np
import pytest

import phase_gray as pg
from helpers import TorchMem, c_params
from test_emu_opencv_build import _RZ_ENV

pytestmark = pytest.mark.gpu

FLOAT_TOL, U8_MAX, U8_FRAC = 1e-4, 1, 0.999            # the parity bar of the BGR Riesz tests
STRIPS = {"LVM_RZ_COLLAPSE_STRIPS_MIN": "1"}


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


def _env(monkeypatch, env):
    for k in _RZ_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bgr_frames(lvm, ctx, dev, streams, pk, calls):
    """the BGR path on the expanded clips: (produced flags, outputs [n][stream][h][w][3]); calls=None: lvm_process_device per frame"""
    fin = pg.expand(np.stack(streams, axis=1))                        # [n][stream][h][w][3]
    n, S, h, w, _ = fin.shape
    fb = w * h * 3
    d_in = dev.upload(fin)
    d_out = dev.zeros_like(d_in)
    prod, t = [], 0
    for nf in calls or (1,) * n:
        if calls is None:
            prod.append(ctx.process_device(c_params(lvm, pk), dev.ptr(d_in, t), w, h, 3, w * 3, fb, dev.ptr(d_out, t), w * 3, fb, dev.stream()))
        else:
            prod += ctx.process_device_frames(c_params(lvm, pk), nf, dev.ptr(d_in, t), w, h, 3, w * 3, fb, fb * S, dev.ptr(d_out, t), w * 3, fb, fb * S, dev.stream())
        t += nf
    dev.sync(ctx)
    return prod, dev.download(d_out)


def _gray_frames(lvm, ctx, dev, streams, pk, calls):
    if calls is not None:
        return pg.run_frames(lvm, ctx, dev, streams, pk, calls)
    fin = np.stack(streams, axis=1)
    n, S, h, w = fin.shape
    d_in = dev.upload(fin)
    d_out = dev.zeros_like(d_in)
    prod = [ctx.process_device(c_params(lvm, pk), dev.ptr(d_in, t), w, h, 1, w, w * h, dev.ptr(d_out, t), w, w * h, dev.stream()) for t in range(n)]
    dev.sync(ctx)
    return prod, dev.download(d_out)


@pytest.mark.parametrize("sched", ["per_frame", "batches", "two_streams", "strips", "strips_two_streams"])
@pytest.mark.parametrize("w,h,levels", pg.SHAPES)
def test_gray_equals_the_bgr_path_on_the_expanded_clip(lvm, po, hip, dev, w, h, levels, sched, monkeypatch):
    _env(monkeypatch, STRIPS if sched.startswith("strips") else {})
    pk = pg.params(lvm, w, h, levels)
    streams = [pg.gray_clip(lvm, po, w, h, levels)]
    if sched.endswith("two_streams"):
        streams.append(pg.gray_clip(lvm, po, w, h, levels, seed=1235))
    calls = None if sched == "per_frame" else pg.CALLS
    gray = pg.context(lvm, hip, len(streams), "default", keep_float=False)
    bgr = pg.context(lvm, hip, len(streams), "default", keep_float=False, on=False)
    try:
        if sched.startswith("strips"):
            gray.profile(True)
        pg_, og = _gray_frames(lvm, gray, dev, streams, pk, calls)
        pb, ob = _bgr_frames(lvm, bgr, dev, streams, pk, calls)
        assert pg_ == pb and sum(pg_) >= pg.NFRAMES - 1, (pg_, pb)
        for t in range(pg.NFRAMES):
            for s in range(len(streams)):
                if not pg_[t]:
                    continue
                want = po.bgr2gray_u8(ob[t, s])
                assert np.array_equal(og[t, s], want), "frame %d stream %d: %d bytes differ from the BGR path" % (t, s, int((og[t, s] != want).sum()))
                assert float((og[t, s] != streams[s][t]).mean()) > 0.5                       # (and it is not the input)
        if sched.startswith("strips") and w % 4 == 0:
            assert gray.profile_variants()["rz_final"] == {"gray-strips"}
    finally:
        gray.close(); bgr.close()


@pytest.mark.parametrize("env", [{}, STRIPS], ids=["default", "strips"])
@pytest.mark.parametrize("w,h,levels", pg.SHAPES)
def test_gray_phase_meets_the_parity_bar(lvm, po, hip, dev, w, h, levels, env, monkeypatch):
    """shipped configuration for the bytes, a float-keeping context of the same flavour for the float frame (it selects the DBG builds
    of the output kernels), both against the oracle on the expanded frames"""
    _env(monkeypatch, env)
    frames, pk = pg.gray_clip(lvm, po, w, h, levels), pg.params(lvm, w, h, levels)
    refs = pg.clip_reference(lvm, po, w, h, levels, 0)
    pg.assert_not_vacuous(frames, refs)
    worst = [0.0, 0, 1.0]
    ship = pg.context(lvm, hip, 1, "default", keep_float=False)
    keep = pg.context(lvm, hip, 1, "default", keep_float=True)
    try:
        prod, outs = pg.run_frames(lvm, ship, dev, [frames], pk)
        assert prod == [r[0] for r in refs], prod
        for t, (pr, gray, _) in enumerate(refs):
            if pr:
                du = np.abs(gray.astype(np.int32) - outs[t, 0].astype(np.int32))
                worst[1:] = [max(worst[1], int(du.max())), min(worst[2], float((du == 0).mean()))]
        d_in = dev.upload(np.array(frames))
        d_out = dev.zeros_like(d_in)
        for t in range(pg.NFRAMES):                                   # lvm_process_device: the float frame of every frame
            p = keep.process_device(c_params(lvm, pk), dev.ptr(d_in, t), w, h, 1, w, w * h, dev.ptr(d_out, t), w, w * h, dev.stream())
            dev.sync(keep)
            assert p == refs[t][0], t
            if p:
                fr, fg = refs[t][2], keep.read_float((h, w, 3))
                assert np.isfinite(fg).all()
                worst[0] = max(worst[0], float(np.abs(fr - fg).max() / np.abs(fr).max()))
                du = np.abs(refs[t][1].astype(np.int32) - dev.download(d_out)[t].astype(np.int32))
                worst[1:] = [max(worst[1], int(du.max())), min(worst[2], float((du == 0).mean()))]
    finally:
        ship.close(); keep.close()
    print("HIP gray Phase vs oracle(expand) -> BGR2GRAY, cfg2 %dx%d L%d %s: float %.2e  u8 max %d  identical %.5f" % (
        w, h, levels, "strips" if env else "default", worst[0], worst[1], worst[2]))
    assert worst[0] <= FLOAT_TOL and worst[1] <= U8_MAX and worst[2] >= U8_FRAC, worst


def test_the_launch_code_picks_the_gray_kernels(lvm, po, hip, dev, monkeypatch):
    """lvm_profile_variants: dword forms on 264 x 150 (the strip kernel where the switch sends level 0 to it), byte forms on 67 x 131,
    and no (ia, ib) plane kernel anywhere"""
    seen = {}
    for key, (w, h, levels), env in (("vec", (264, 150, 3), {}), ("strips", (264, 150, 3), STRIPS), ("bytes", (67, 131, 2), {})):
        _env(monkeypatch, env)
        ctx = pg.context(lvm, hip, 1, "default", keep_float=False)
        ctx.profile(True)
        try:
            pg.run_frames(lvm, ctx, dev, [pg.gray_clip(lvm, po, w, h, levels)], pg.params(lvm, w, h, levels))
            v = ctx.profile_variants()
            seen[key] = {n: v.get(n, set()) for n in ctx.profile_collect()}
        finally:
            ctx.close()
    assert seen["vec"]["lab_lut"] == {"gray4"} and seen["vec"]["rz_final"] == {"gray4"}, seen["vec"]
    assert seen["strips"]["lab_lut"] == {"gray4"} and seen["strips"]["rz_final"] == {"gray-strips"}, seen["strips"]
    assert seen["bytes"]["lab_lut"] == {"gray"} and seen["bytes"]["rz_final"] == {"gray"}, seen["bytes"]
