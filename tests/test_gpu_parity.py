"""Parity tests proper: the gfx950 library (liblvm_hip.so) through the C ABI vs the CPU oracle
on the same seeded synthetic clips.  Tolerances (BASELINE.json north_star):
float frame max|d|/max|ref| <= 1e-4, u8 frame <= 1 LSB with >= 99.9 % identical pixels,
produced flags identical frame by frame."""
import numpy as np
import pytest

import parity_matrix as M
from helpers import c_params, run_pair

pytestmark = pytest.mark.gpu

FLOAT_TOL = 1e-4


@pytest.mark.parametrize("w,h,levels,ch", [(640, 360, 4, 3), (135, 77, 4, 3), (100, 64, 2, 1), (64, 48, 1, 3),
                                            (323, 211, 5, 3)])
def test_laplace_small(lvm, po, hip, w, h, levels, ch):
    ck, pk = lvm.synth.config(0, (w, h, levels))
    ck["channels"] = ch
    clip = lvm.synth.Clip(**ck)
    worst = run_pair(lvm, po, hip, clip, pk, 24 if w >= 640 else 10, FLOAT_TOL)
    print("laplace", (w, h, levels, ch), "worst rel/u8/frac", worst)
    run_pair(lvm, po, hip, clip, pk, 24 if w >= 640 else 10, 0.0, exact=True)     # the exact flavour: bit for bit (test_gpu_exact.py)


def test_laplace_cfg0_64_frames(lvm, po, hip):
    """BASELINE.json configs[0]: 640x360, 4 levels, IIR 0.4-3 Hz (state drift included)."""
    ck, pk = lvm.synth.config(0)
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 64, FLOAT_TOL)
    print("cfg0 worst", worst)


def test_laplace_1080p_full_size(lvm, po, hip):
    """BASELINE.json configs[1] at full size: direct parity on a few frames plus size-independent
    properties (first frame = Lab round trip, static clip => no motion, reset => replay)."""
    ck, pk = lvm.synth.config(1)
    clip = lvm.synth.Clip(**ck)
    worst = run_pair(lvm, po, hip, clip, pk, 5, FLOAT_TOL)
    print("1080p worst", worst)
    ctx = lvm.Context(0, 1, hip)
    cp = c_params(lvm, pk)
    f0 = clip.frame(0)
    out0, prod = ctx.process(f0, cp)
    assert prod and np.abs(out0.astype(int) - f0.astype(int)).max() <= 1
    outs = [ctx.process(clip.frame(t), cp)[0].copy() for t in range(1, 4)]
    ctx.reset()
    ctx.process(f0, cp)
    again = [ctx.process(clip.frame(t), cp)[0].copy() for t in range(1, 4)]
    for a, b in zip(outs, again):
        assert np.array_equal(a, b)
    static = lvm.synth.Clip(**dict(ck, amp_px=0.0))
    ctx.reset()
    for t in range(4):
        f = static.frame(t)
        out, _ = ctx.process(f, cp)
        assert np.abs(out.astype(int) - f.astype(int)).max() <= 1
    ctx.close()


def test_laplace_param_change_and_reset(lvm, po, hip):
    ck, pk = lvm.synth.config(0, (320, 180, 4))

    def vary(t, p):
        if t >= 4:
            p["amplification"] = 35.0; p["coLow"] = 0.0
        if t >= 8:
            p["levels"] = 2
        return p
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 12, FLOAT_TOL, param_fn=vary)


def test_laplace_batched_streams_device_path(lvm, po, hip):
    """n_streams = 3 through lvm_process_device on device memory (torch tensors)."""
    import torch
    ck, pk = lvm.synth.config(0, (320, 180, 4))
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(3)]
    h, w = 180, 320
    ctx = lvm.Context(0, 3, hip)
    orcs = [po.Oracle() for _ in range(3)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    stream = torch.cuda.current_stream().cuda_stream
    for t in range(8):
        fin = np.stack([c.frame(t) for c in clips])
        d_in = torch.from_numpy(fin).cuda()
        d_out = torch.zeros_like(d_in)
        assert ctx.process_device(cp, d_in.data_ptr(), w, h, 3, w * 3, w * h * 3, d_out.data_ptr(), w * 3, w * h * 3, stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for s in range(3):
            ref, _ = orcs[s].process(fin[s], P)
            du = np.abs(ref.astype(int) - got[s].astype(int))
            assert du.max() <= 1 and (du == 0).mean() >= 0.999
    ctx.close()


@pytest.mark.parametrize("idx,pad_in,pad_out", [(0, 4, 8), (0, 1, 3), (2, 4, 4), (2, 7, 1), (3, 8, 4), (3, 5, 5)])
def test_padded_row_strides_device_path(lvm, po, hip, idx, pad_in, pad_out):
    """Ragged rows (stride > width * channels, as a cv::Mat ROI view has): dword-aligned paddings keep the
    vectorised kernels, odd ones select the byte kernels; the padding bytes of the output stay untouched."""
    import torch
    w, h, levels = 320, 180, 4
    ck, pk = lvm.synth.config(idx, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, 1, hip)
    orc = po.Oracle()
    si, so = w * 3 + pad_in, w * 3 + pad_out
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for t in range(6):
            f = clip.frame(t)
            buf_in = np.full((h, si), 0xAB, np.uint8)
            buf_in[:, :w * 3] = f.reshape(h, w * 3)
            d_in = torch.from_numpy(buf_in).cuda()
            d_out = torch.full((h, so), 0xCD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ref, pr = orc.process(f, P)
            pg = ctx.process_device(cp, d_in.data_ptr(), w, h, 3, si, si * h, d_out.data_ptr(), so, so * h, stream)
            torch.cuda.synchronize()
            assert pr == pg
            got = d_out.cpu().numpy()
            assert (got[:, w * 3:] == 0xCD).all(), "padding bytes of the output were written"
            if pr:
                du = np.abs(ref.astype(int) - got[:, :w * 3].reshape(h, w, 3).astype(int))
                assert du.max() <= 1 and (du == 0).mean() >= 0.999
    finally:
        ctx.close(); orc.close()


@pytest.mark.parametrize("idx,const_from", [(0, None), (2, None), (3, None), (0, 5), (2, 5), (3, 5)])
def test_flat_regions_and_constant_frames(lvm, po, hip, idx, const_from):
    """Flat black / white blocks and a switch to constant frames: the 0/0 and max == min corners of the three modes."""
    ck, pk = lvm.synth.config(idx, (320, 180, 4))
    if idx == 3:
        ck["fps"] = 15.0; pk["framerate"] = 15.0
    base = lvm.synth.Clip(**ck)

    class Patched:
        def frame(self, t):
            f = base.frame(t).copy()
            h, w = f.shape[:2]
            f[h // 8:h // 2, w // 8:w // 3] = 0
            f[h // 2:h - h // 8, w // 2:w - w // 8] = 255
            if const_from is not None and t >= const_from:
                f[...] = 77
            return f
    run_pair(lvm, po, hip, Patched(), pk, 9, FLOAT_TOL)


@pytest.mark.parametrize("idx", [0, 2, 3])
def test_fully_constant_clip(lvm, po, hip, idx):
    """Every frame the same constant: Color's output range collapses (max == min), Riesz sees 0/0 everywhere."""
    ck, pk = lvm.synth.config(idx, (320, 180, 4))
    if idx == 3:
        pk["framerate"] = 15.0

    class Const:
        f = np.full((180, 320, 3), 131, np.uint8)

        def frame(self, t):
            return self.f
    run_pair(lvm, po, hip, Const(), pk, 8, FLOAT_TOL)


@pytest.mark.parametrize("idx,over", [(3, dict(coLow=5.0, coHigh=1.0)), (3, dict(coLow=0.0, coHigh=0.3)), (2, dict(coLow=0.5, coHigh=20.0)),
                                       (2, dict(coLow=0.5, coHigh=15.0)), (2, dict(coLow=3.0, coHigh=1.0)),
                                       (0, dict(amplification=1000.0, chromAttenuation=1.0)), (0, dict(amplification=0.0)),
                                       (2, dict(amplification=0.0, coWavelength=0.0))])
def test_extreme_parameters(lvm, po, hip, idx, over):
    """Empty / degenerate pass bands, cutoffs at and above Nyquist, zero and huge gains (see the emulation test of the same name)."""
    ck, pk = lvm.synth.config(idx, (320, 180, 4))
    if idx == 3:
        ck["fps"] = 15.0; pk["framerate"] = 15.0
    pk.update(over)
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 8, FLOAT_TOL)


@pytest.mark.parametrize("idx,frames", [(0, 600), (2, 400), (3, 400)])
def test_long_clip_state_drift(lvm, po, hip, idx, frames):
    """Hundreds of frames: the IIR / Butterworth / rolling-window states of the default (fast) arithmetic must not drift
    away from the oracle's (parity metric of SURVEY.md 8c: >= 64 frames, state drift included)."""
    ck, pk = lvm.synth.config(idx, (160, 90, 3))
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, frames, FLOAT_TOL)
    print("long clip mode", idx, "frames", frames, "worst rel/u8/frac", worst)


def test_passthrough_and_errors(lvm, po, hip):
    ctx = lvm.Context(0, 1, hip)
    f = np.full((40, 40, 3), 90, np.uint8)
    out, produced = ctx.process(f, lvm.LvmParams(3, 4, 0, 0, 0, 0, 0, 30.0, 0))
    assert not produced
    tiny = np.full((5, 40, 3), 90, np.uint8)
    _, produced = ctx.process(tiny, lvm.LvmParams(0, 4, 10, 100, 0.1, 0.4, 0, 30.0, 0))
    assert not produced
    with pytest.raises(lvm.LvmError):
        ctx.process(np.zeros((32, 32, 2), np.uint8), lvm.LvmParams(0, 2, 10, 100, 0.1, 0.4, 0, 30.0, 0))
    ctx.reset()                                    # the context keeps working after an error
    _, produced = ctx.process(np.full((64, 64, 3), 7, np.uint8), lvm.LvmParams(0, 2, 10, 100, 0.1, 0.4, 0, 30.0, 0))
    assert produced
    ctx.close()


# ---- Riesz (phase) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", [(320, 180, 4), (135, 77, 4), (64, 48, 1), (323, 211, 5)])
def test_riesz_small(lvm, po, hip, w, h, levels):
    ck, pk = lvm.synth.config(2, (w, h, levels))
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 24, FLOAT_TOL)
    print("riesz", (w, h, levels), "worst rel/u8/frac", worst)


def test_riesz_64_frames_state_drift(lvm, po, hip):
    ck, pk = lvm.synth.config(2, (640, 360, 5))
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 64, FLOAT_TOL)
    print("riesz 640x360 L5 64 frames worst", worst)


def test_riesz_1080p_full_size(lvm, po, hip):
    """BASELINE.json configs[2] at full size, a few frames (the oracle needs ~0.5 s per frame)."""
    ck, pk = lvm.synth.config(2)
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 5, FLOAT_TOL)
    print("riesz 1080p worst", worst)


def test_riesz_4k_8_levels_configs4(lvm, po, hip):
    """BASELINE configs[4]'s per-GPU share at its full size (3840x2160, 8 levels): a few frames against the oracle,
    per-frame calls and one temporal batch of the same stream."""
    import torch
    ck, pk = lvm.synth.config(4)
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 3, FLOAT_TOL)
    print("riesz 4K worst", worst)
    clip = lvm.synth.Clip(**ck)
    w, h = ck["w"], ck["h"]
    frames = np.stack([clip.frame(t) for t in range(5)])
    ctx = lvm.Context(0, 1, hip)
    orc = po.Oracle()
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    try:
        d_in = torch.from_numpy(frames).cuda()
        d_out = torch.zeros_like(d_in)
        fb = w * h * 3
        st = torch.cuda.current_stream().cuda_stream
        prod = ctx.process_device_frames(cp, 5, d_in.data_ptr(), w, h, 3, w * 3, fb, fb, d_out.data_ptr(), w * 3, fb, fb, st)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for t in range(5):
            ref, pr = orc.process(frames[t], P)
            assert pr == prod[t]
            if pr:
                du = np.abs(ref.astype(int) - got[t].astype(int))
                assert du.max() <= 1 and (du == 0).mean() >= 0.999, (t, du.max(), (du == 0).mean())
    finally:
        ctx.close(); orc.close()


def test_riesz_cutoff_change(lvm, po, hip):
    ck, pk = lvm.synth.config(2, (320, 180, 4))

    def vary(t, p):
        if t >= 4:
            p["coLow"] = 1.0
        if t >= 7:
            p["coHigh"] = 5.0
        return p
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 12, FLOAT_TOL, param_fn=vary)


# ---- Colour ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels,ch,fps", [(320, 180, 4, 3, 60.0), (135, 77, 3, 3, 30.0), (67, 131, 2, 1, 15.0)])
def test_color_small(lvm, po, hip, w, h, levels, ch, fps):
    ck, pk = lvm.synth.config(3, (w, h, levels))
    ck["channels"] = ch; ck["fps"] = fps; pk["framerate"] = fps
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 40, FLOAT_TOL)
    print("color", (w, h, levels, ch, fps), "worst", worst)
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 40, 0.0, exact=True)       # the exact flavour: bit for bit (test_gpu_exact.py)


@pytest.mark.parametrize("rows", ["4", "17"])
@pytest.mark.parametrize("w,h,levels", [(320, 180, 4), (264, 90, 3), (520, 77, 3)])
def test_color_two_level_first_pass_on_the_gpu(lvm, po, hip, w, h, levels, rows, monkeypatch):
    """k_down01_rows (production: launches of >= 4096 strips) forced onto small frames on the GPU: strip heights, an odd number of
    level-1 rows (77 -> 39), several strips per row; and k_col_out_strips on the same frames (bit-exactness is the emulation suite's
    job, this is the hardware run of the same code: DPP, ds_bpermute, buffer loads / stores, constant-address-space tables)."""
    monkeypatch.setenv("LVM_D0_MIN_TASKS", "0")
    monkeypatch.setenv("LVM_COL_DOWN01_ROWS", rows)
    monkeypatch.setenv("LVM_COL_OUT_MIN_TASKS", "0")
    ck, pk = lvm.synth.config(3, (w, h, levels))
    ck["fps"] = 15.0; pk["framerate"] = 15.0
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 24, FLOAT_TOL)


def test_color_previous_strip_kernels_on_the_gpu(lvm, po, hip, monkeypatch):
    """LVM_COL_OUT_LEAN=0: k_col_out_rows (fallback of k_col_out_strips) still matches."""
    monkeypatch.setenv("LVM_COL_OUT_LEAN", "0")
    monkeypatch.setenv("LVM_COL_OUT_MIN_TASKS", "0")
    ck, pk = lvm.synth.config(3, (320, 180, 4))
    ck["fps"] = 15.0; pk["framerate"] = 15.0
    run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 24, FLOAT_TOL)


def test_color_1080p_window_fill(lvm, po, hip):
    """BASELINE.json configs[3] geometry (1080p, 6 levels, fps 60 => T = 128): run past the point
    where the window is full and starts rolling."""
    ck, pk = lvm.synth.config(3)
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 134, FLOAT_TOL)
    print("color 1080p worst", worst)


# ---- chromatic content (tests/content.py) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,idx,w,h,levels", M.CHROMA_CASES)
def test_chroma_default_flavour(lvm, po, hip, kind, idx, w, h, levels):
    """Saturated colours through the default flavour (float32 cube root, reciprocal multiplies, packed Lab2BGR) of every mode, and
    through the shipped configuration's step table (run_pair's second context)."""
    worst = M.chroma_shape(lvm, po, hip, kind, idx, w, h, levels, flavour_exact=False)
    print("chroma default flavour", kind, (idx, w, h, levels), "worst rel/u8/frac, shipped u8/frac", worst)


@pytest.mark.parametrize("kind,idx,w,h,levels", [c for c in M.CHROMA_CASES if c[1] == 2])
def test_chroma_riesz_exact_flavour(lvm, po, hip, kind, idx, w, h, levels):
    """Riesz in OpenCV's operation order: the bars, not bit-equality (device acosf / sinf / cosf; Laplace and Color: test_gpu_exact.py)"""
    worst = M.chroma_shape(lvm, po, hip, kind, idx, w, h, levels, flavour_exact=True, bit_exact=False)
    print("chroma riesz exact flavour", kind, (w, h, levels), "worst rel/u8/frac, shipped u8/frac", worst)


# ---- cross-frame pipeline ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", [(640, 360, 4), (1920, 1080, 6)])
def test_laplace_pipelined_device_path(lvm, po, hip, w, h, levels):
    """lvm_process_device at pipeline depth 1 (stage B of frame t+1 on a second stream, concurrent
    with stage A of frame t) over a ring of device buffers; outputs must match the oracle."""
    import torch
    ck, pk = lvm.synth.config(0, (w, h, levels))
    clip = lvm.synth.Clip(**ck)
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ring, nframes = 4, 22 if w < 1000 else 10
    ctx = lvm.Context(0, 1, hip)
    ctx.set_pipeline(1)
    orc = po.Oracle()
    d_in = torch.zeros((ring, h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros_like(d_in)
    stream = torch.cuda.current_stream().cuda_stream
    refs = {}

    def check(t):
        got = d_out[t % ring].cpu().numpy()
        du = np.abs(refs[t].astype(int) - got.astype(int))
        assert du.max() <= 1 and (du == 0).mean() >= 0.999, "frame %d: max %d, identical %.5f" % (t, du.max(), (du == 0).mean())

    for t in range(nframes):
        k = t % ring
        if t >= ring:
            torch.cuda.synchronize()
            check(t - ring)
        f = clip.frame(t)
        refs[t], _ = orc.process(f, P)
        d_in[k].copy_(torch.from_numpy(f).cuda())
        assert ctx.process_device(cp, d_in[k].data_ptr(), w, h, 3, w * 3, w * h * 3, d_out[k].data_ptr(), w * 3, w * h * 3, stream)
    ctx.flush(stream)
    torch.cuda.synchronize()
    for t in range(nframes - ring, nframes):
        check(t)
    ctx.close()


@pytest.mark.parametrize("w,h,levels,ns,nf", [(640, 360, 4, 1, 8), (1920, 1080, 6, 1, 6), (640, 360, 4, 2, 5)])
def test_laplace_temporal_batches_device(lvm, po, hip, w, h, levels, ns, nf):
    """lvm_process_device_frames on device memory: batches of nf consecutive frames."""
    import torch
    ck, pk = lvm.synth.config(0, (w, h, levels))
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(ns)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, ns, hip)
    orcs = [po.Oracle() for _ in range(ns)]
    stream = torch.cuda.current_stream().cuda_stream
    fb = w * h * 3
    t = 0
    for call in range(3):
        fin = np.stack([np.stack([c.frame(t + f) for c in clips]) for f in range(nf)])
        d_in = torch.from_numpy(fin).cuda()
        d_out = torch.zeros_like(d_in)
        produced = ctx.process_device_frames(cp, nf, d_in.data_ptr(), w, h, 3, w * 3, fb, fb * ns, d_out.data_ptr(), w * 3, fb, fb * ns, stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for f in range(nf):
            for s_ in range(ns):
                ref, pr = orcs[s_].process(fin[f, s_], P)
                assert produced[f] == pr
                du = np.abs(ref.astype(int) - got[f, s_].astype(int))
                assert du.max() <= 1 and (du == 0).mean() >= 0.999, (t + f, s_, du.max(), (du == 0).mean())
        t += nf
    ctx.close()


@pytest.mark.parametrize("w,h,levels,ns,nf", [(640, 360, 5, 1, 8), (1920, 1080, 6, 1, 4), (320, 180, 4, 2, 5)])
def test_riesz_temporal_batches_device(lvm, po, hip, w, h, levels, ns, nf):
    import torch
    ck, pk = lvm.synth.config(2, (w, h, levels))
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(ns)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, ns, hip)
    orcs = [po.Oracle() for _ in range(ns)]
    stream = torch.cuda.current_stream().cuda_stream
    fb = w * h * 3
    t = 0
    for call in range(3):
        fin = np.stack([np.stack([c.frame(t + f) for c in clips]) for f in range(nf)])
        d_in = torch.from_numpy(fin).cuda()
        d_out = torch.zeros_like(d_in)
        produced = ctx.process_device_frames(cp, nf, d_in.data_ptr(), w, h, 3, w * 3, fb, fb * ns, d_out.data_ptr(), w * 3, fb, fb * ns, stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for f in range(nf):
            for s_ in range(ns):
                ref, pr = orcs[s_].process(fin[f, s_], P)
                assert produced[f] == pr
                if pr:
                    du = np.abs(ref.astype(int) - got[f, s_].astype(int))
                    assert du.max() <= 1 and (du == 0).mean() >= 0.999, (t + f, s_, du.max(), (du == 0).mean())
        t += nf
    ctx.close()


@pytest.mark.parametrize("w,h,levels,ns,calls", [(320, 180, 4, 2, (34, 8, 13, 5)), (1920, 1080, 6, 2, (34, 32))])
def test_color_temporal_batches_device(lvm, po, hip, w, h, levels, ns, calls):
    """Colour mode, fps 15 (window of 32 columns): per-frame until the window is full, then batches.  The 1080p case is the production
    shape of the round-3 kernels: two streams x 32 frames per launch take k_down01_rows unforced and k_col_out_strips with 36-row strips."""
    import torch
    ck, pk = lvm.synth.config(3, (w, h, levels))
    ck["fps"] = 15.0; pk["framerate"] = 15.0; pk["coLow"] = 0.5; pk["coHigh"] = 2.0
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(ns)]
    P = po.make_params(**pk)
    cp = c_params(lvm, pk)
    ctx = lvm.Context(0, ns, hip)
    orcs = [po.Oracle() for _ in range(ns)]
    stream = torch.cuda.current_stream().cuda_stream
    fb = w * h * 3
    t = 0
    for nf in calls:
        fin = np.stack([np.stack([c.frame(t + f) for c in clips]) for f in range(nf)])
        d_in = torch.from_numpy(fin).cuda()
        d_out = torch.zeros_like(d_in)
        produced = ctx.process_device_frames(cp, nf, d_in.data_ptr(), w, h, 3, w * 3, fb, fb * ns, d_out.data_ptr(), w * 3, fb, fb * ns, stream)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        for f in range(nf):
            for s_ in range(ns):
                ref, pr = orcs[s_].process(fin[f, s_], P)
                assert produced[f] == pr, (t + f, produced[f], pr)
                if pr:
                    du = np.abs(ref.astype(int) - got[f, s_].astype(int))
                    assert du.max() <= 1 and (du == 0).mean() >= 0.999, (t + f, s_, du.max(), (du == 0).mean())
        t += nf
    ctx.close()


@pytest.mark.parametrize("idx,size", [(0, (640, 360, 4)), (2, (320, 180, 4)), (0, (323, 211, 5))])
def test_analytic_flavour_on_the_gpu(lvm, po, hip, idx, size):
    """lvm_debug_lab_analytic (OpenCV with its Lab interpolation switched off; implies OpenCV's operation order) against the
    oracle in the same mode, at the usual bars."""
    ck, pk = lvm.synth.config(idx, size)
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 12, FLOAT_TOL, analytic=True)
    print("analytic flavour", idx, size, worst)


def test_lab_table_of_the_gpu_library_equals_the_oracles(lvm, po, hip):
    t = np.empty(33 * 33 * 33 * 3, np.int16)
    po.lib().lvmo_lab_lut_table(t.ctypes.data)
    ctx = lvm.Context(0, 1, hip)
    try:
        assert np.array_equal(ctx.lab_lut(), t)
    finally:
        ctx.close()


def test_variant_envelope_gpu(lvm, po, hip):
    """The HIP column of DESIGN.md section 5's envelope table (tests/test_oracle_variants.py has the oracle's): the gfx950
    library (default flavour) against the oracle under each unpinned OpenCV build choice, BASELINE configs 0 / 2 / 3 at 320 x 180
    over 64 frames.  Asserted: against the DEFAULT restatement the library is inside the bar; against every build-choice
    variant of Laplace and Color too (those modes are well-conditioned: whichever dispatch a maintainer's OpenCV takes, the
    drop-in claim holds); for Riesz and for the forward-table residuals the distances are printed (`-s`) and only
    sanity-bounded -- they are the oracle's own distance to that variant, to which the library adds ~4e-6."""
    sizes = {0: (320, 180, 4), 2: (320, 180, 5), 3: (320, 180, 4)}
    applies = {0: ["pyr_simd", "addw_fused", "gamma_f32", "lut_nudge_up", "lut_nudge_down", "spline_cv3"],
               2: ["filter_unfused", "filter_dft", "mul_f32", "gamma_f32", "lut_nudge_up", "lut_nudge_down", "spline_cv3"], 3: ["pyr_simd", "dft_f32"]}
    build_choices = ("pyr_simd", "filter_unfused", "filter_dft", "addw_fused", "mul_f32", "dft_f32")
    nframes = {0: 64, 2: 64, 3: 150}      # colour: past its 128-frame window (the power-of-two transform length)
    for cfg in (0, 2, 3):
        ck, pk = lvm.synth.config(cfg, sizes[cfg])
        clip = lvm.synth.Clip(**ck)
        frames = [clip.frame(t) for t in range(nframes[cfg])]
        cp = c_params(lvm, pk)
        ctx = lvm.Context(0, 1, hip)
        ctx.keep_float(True)
        got = []
        for f in frames:
            out, pg = ctx.process(f, cp)
            got.append((ctx.read_float(f.shape).copy(), out.copy()) if pg else None)
        ctx.close()
        for name in ["default"] + applies[cfg]:
            po.set_variant(0 if name == "default" else po.VARIANTS[name])
            orc = po.Oracle()
            P = po.make_params(**pk)
            rel, du, same = 0.0, 0, 1.0
            try:
                for f, g in zip(frames, got):
                    ref, pr = orc.process(f, P)
                    assert pr == (g is not None)
                    if not pr:
                        continue
                    fr = orc.last_float()
                    rel = max(rel, float(np.abs(fr - g[0]).max() / np.abs(fr).max()))
                    d = np.abs(ref.astype(np.int32) - g[1].astype(np.int32))
                    du = max(du, int(d.max())); same = min(same, float((d == 0).mean()))
            finally:
                orc.close()
                po.set_variant(0)
            print("HIP vs oracle[%-15s] cfg%d  float %.2e  u8 max %d  identical %.5f" % (name, cfg, rel, du, same))
            if name == "default" or (cfg != 2 and name in build_choices):
                assert rel <= FLOAT_TOL and du <= 1 and same >= 0.999, (cfg, name, rel, du, same)
            else:
                assert rel <= 5e-3 and du <= 3 and same >= 0.99, (cfg, name, rel, du, same)
