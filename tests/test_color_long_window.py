"""Color mode at the window lengths of high-speed footage (1025..4096 frames: capture rates up to 2048 fps): k_col_dft_long, its temporal
batches and the twiddle table that is refilled, not reallocated, while the window fills.  Every comparison is byte equality.

A. Small windows forced onto the long-window kernel (LVM_COL_LONG_FROM=2) against the live oracle: every warm-up length 2..16, odd and
   even, half-passed / Nyquist / DC entries, a band of 75 entries, batches (also behind a wrapped ring), two streams, a falling
   framerate.  LVM_COL_LONG_DFT=0 sends the same windows through the serial kernel, frame by frame: the same bytes.
B. True sizes (windows of 2048 and 4096 frames) against frames the oracle produced once (tests/golden/make_color_long.py ->
   tests/golden/color_long_window.npz: the oracle's filter costs minutes at these lengths).  Frames: 6 x 6 gray, 1 level; frame t, pixel
   i = y * 6 + x: 4 + (((t * 36 + i) * 1103515245 + 12345) >> 16) % 248.
"""
import functools
import json
import os

import numpy as np
import pytest

from helpers import HostMem, TorchMem, c_params, frames_clip

HOST = HostMem()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_long_window.npz")


@pytest.fixture(scope="module")
def dev():
    return TorchMem()


def _launches(ctx, name="col_dft"):
    return ctx.profile_collect().get(name, (0.0, 0))[1]


# ---- A: forced small windows against the live oracle ---------------------------------------------------------------------------
A_SIZE = (40, 30, 2)


@functools.lru_cache(maxsize=None)
def _a_frames(lvm, n):
    ck, _ = lvm.synth.config(3, A_SIZE)
    return lvm.synth.Clip(**ck).frames(n)


def _a_params(lvm, fps, band):
    _, pk = lvm.synth.config(3, A_SIZE)
    pk.update(framerate=float(fps), coLow=band[0], coHigh=band[1])
    return pk


def _a_plan(lvm, calls, fps, band, change=None):
    """[(frames of the call, parameters)]; change = (frame, fps): the framerate from the call that starts at that frame on"""
    plan, t = [], 0
    for nf in calls:
        plan.append((nf, _a_params(lvm, change[1] if change and t >= change[0] else fps, band)))
        t += nf
    assert change is None or change[0] in np.cumsum([0] + list(calls))
    return plan


@functools.lru_cache(maxsize=None)
def _a_reference(lvm, po, calls, fps, band, change=None):
    """the oracle over the frames of a plan, computed once per case and shared by the builds and switches that run it"""
    frames = _a_frames(lvm, sum(calls))
    orc = po.Oracle()
    prod, out, t = [], np.zeros_like(frames), 0
    try:
        for nf, pk in _a_plan(lvm, calls, fps, band, change):
            P = po.make_params(**pk)
            for f in range(t, t + nf):
                ref, pr = orc.process(frames[f], P)
                prod.append(bool(pr))
                if pr:
                    out[f] = ref
            t += nf
    finally:
        orc.close()
    out.setflags(write=False)
    return prod, out


def _a_run(lvm, lib, mem, calls, fps, band, change=None):
    """one context through the calls of a plan (lvm_process_device_frames), profiled: (produced flags, frames, variants of col_dft,
    col_dft launches of each call)"""
    w, h, _ = A_SIZE
    frames = _a_frames(lvm, sum(calls))
    fb = w * h * 3
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.profile(True)
        ctx.profile_only("col_dft")
        d_in = mem.upload(frames)
        d_out = mem.zeros_like(d_in)
        prod, per_call, t = [], [], 0
        for nf, pk in _a_plan(lvm, calls, fps, band, change):
            before = _launches(ctx)
            prod += ctx.process_device_frames(c_params(lvm, pk), nf, mem.ptr(d_in, t), w, h, 3, w * 3, fb, fb, mem.ptr(d_out, t), w * 3, fb, fb,
                                              mem.stream())
            per_call.append(_launches(ctx) - before)
            t += nf
        mem.sync(ctx)
        out = np.array(mem.download(d_out), copy=True)
        out[~np.asarray(prod, bool)] = 0
        return prod, out, ctx.profile_variants().get("col_dft", set()), per_call
    finally:
        ctx.close()


def _a_check(lvm, po, lib, mem, calls, fps, band, change=None):
    prod_r, out_r = _a_reference(lvm, po, tuple(calls), fps, band, change)
    prod, out, variants, per_call = _a_run(lvm, lib, mem, calls, fps, band, change)
    assert prod == prod_r, [t for t, (a, b) in enumerate(zip(prod, prod_r)) if a != b]
    assert any(prod_r)
    bad = [(t, int((out[t] != out_r[t]).sum())) for t in range(len(prod)) if not np.array_equal(out[t], out_r[t])]
    assert not bad, "(frame, bytes that differ from the oracle): %s" % bad[:8]
    return variants, per_call


# window 16 (fps 7): every warm-up length 2..16; (2.9, 3.5) passes a half-passed bin and the Nyquist entry, (0.0, 40.0) everything but
# DC, (-0.5, 1.2) the DC entry (a cutoff of 0 is raised to 0.01 Hz: only a negative one lets element 0 through).  The last case goes
# on until the ring of 64 slots has wrapped under the batches.
A16_CALLS = (18, 5, 7, 9)
A16 = [(A16_CALLS, (0.8, 1.6)), (A16_CALLS, (2.9, 3.5)), (A16_CALLS, (0.0, 40.0)), (A16_CALLS, (-0.5, 1.2)), ((18, 5, 7, 9, 32, 9), (0.8, 1.6))]
A256_CALLS = (258, 32, 7)          # window 256 (fps 120), band (5, 40): 75 entries, each owned by a thread; the inverse walks them all


def _a16(lvm, po, lib, mem, monkeypatch, calls, band):
    monkeypatch.setenv("LVM_COL_LONG_FROM", "2")
    variants, per_call = _a_check(lvm, po, lib, mem, calls, 7, band)
    assert variants == {"long"}, variants
    assert per_call[0] == 16 and per_call[1:] == [1] * (len(calls) - 1), per_call      # 15 warm-up lengths + one batch of 2, then a launch per call


def _a256(lvm, po, lib, mem, monkeypatch):
    monkeypatch.setenv("LVM_COL_LONG_FROM", "2")
    variants, per_call = _a_check(lvm, po, lib, mem, A256_CALLS, 120, (5.0, 40.0))
    assert variants == {"long"}, variants
    assert per_call == [256, 1, 1], per_call                                           # the 32-frame call: ONE col_dft launch


def _a_shrink(lvm, po, lib, mem, monkeypatch):
    """framerate 120 -> 7 at frame 262: the window keeps its 256 columns above the new cap of 16 (one column in, one out per frame),
    the band moves from 2 entries to 30 and the batches end"""
    monkeypatch.setenv("LVM_COL_LONG_FROM", "2")
    variants, per_call = _a_check(lvm, po, lib, mem, (258, 4, 32, 7), 120, (0.8, 1.6), change=(262, 7))
    assert variants == {"long"}, variants
    assert per_call == [256, 1, 32, 7], per_call


def _a_serial(lvm, po, lib, mem, monkeypatch):
    monkeypatch.setenv("LVM_COL_LONG_FROM", "2")
    monkeypatch.setenv("LVM_COL_LONG_DFT", "0")
    for calls, fps, band in ((A16_CALLS, 7, (2.9, 3.5)), (A256_CALLS, 120, (5.0, 40.0))):
        variants, per_call = _a_check(lvm, po, lib, mem, calls, fps, band)
        assert variants == {"serial"}, variants
        assert per_call == [nf if k else nf - 1 for k, nf in enumerate(calls)], per_call   # frame by frame (the first frame has no window yet)


def _a_two_streams(lvm, po, lib, mem, monkeypatch):
    monkeypatch.setenv("LVM_COL_LONG_FROM", "2")
    w, h, levels = A_SIZE
    frames_clip(lvm, po, lib, mem, 3, w, h, levels, 2, A16_CALLS, over=dict(framerate=7.0, coLow=0.8, coHigh=1.6))


@pytest.mark.parametrize("calls,band", A16)
def test_forced_window16_emu(lvm, po, emu, monkeypatch, calls, band):
    _a16(lvm, po, emu, HOST, monkeypatch, calls, band)


def test_forced_window256_emu(lvm, po, emu, monkeypatch):
    _a256(lvm, po, emu, HOST, monkeypatch)


def test_forced_shrinking_framerate_emu(lvm, po, emu, monkeypatch):
    _a_shrink(lvm, po, emu, HOST, monkeypatch)


def test_forced_serial_switch_emu(lvm, po, emu, monkeypatch):
    _a_serial(lvm, po, emu, HOST, monkeypatch)


def test_forced_two_streams_emu(lvm, po, emu, monkeypatch):
    _a_two_streams(lvm, po, emu, HOST, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("calls,band", A16)
def test_forced_window16_gpu(lvm, po, hip, dev, monkeypatch, calls, band):
    _a16(lvm, po, hip, dev, monkeypatch, calls, band)


@pytest.mark.gpu
def test_forced_window256_gpu(lvm, po, hip, dev, monkeypatch):
    _a256(lvm, po, hip, dev, monkeypatch)


@pytest.mark.gpu
def test_forced_shrinking_framerate_gpu(lvm, po, hip, dev, monkeypatch):
    _a_shrink(lvm, po, hip, dev, monkeypatch)


@pytest.mark.gpu
def test_forced_serial_switch_gpu(lvm, po, hip, dev, monkeypatch):
    _a_serial(lvm, po, hip, dev, monkeypatch)


@pytest.mark.gpu
def test_forced_two_streams_gpu(lvm, po, hip, dev, monkeypatch):
    _a_two_streams(lvm, po, hip, dev, monkeypatch)


# ---- B: true sizes against recorded oracle frames -----------------------------------------------------------------------------------
W = H = 6
BASE = {"mode": 2, "levels": 1, "amplification": 50.0, "coWavelength": 0.0, "chromAttenuation": 0.0}
# per clip: framerate, frames, first stored frame, segments (first frame, frame count, frames per call, coLow, coHigh)
CLIPS = {
    "a": {"framerate": 600.0, "frames": 2100, "keep_from": 1000,
          "segments": [[0, 2048, 1, 0.83, 1.0], [2048, 32, 32, 20.0, 45.0], [2080, 8, 8, 0.0, 300.0], [2088, 12, 1, 20.0, 45.0]]},
    "b": {"framerate": 1200.0, "frames": 4130, "keep_from": 4000,
          "segments": [[0, 4096, 1, 1.66, 2.0], [4096, 32, 32, 40.0, 90.0], [4128, 2, 1, 0.0, 600.0]]},
}
SHORT_MAX = 1024            # frame t of a clip sees a window of t + 1 frames: lengths up to this keep the kernels they had


def frame6(t):
    i = np.arange(W * H, dtype=np.int64)
    return (4 + (((t * 36 + i) * 1103515245 + 12345) >> 16) % 248).astype(np.uint8).reshape(H, W)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    par = json.loads(str(g["params"]))
    assert par == {"w": W, "h": H, "base": BASE, "clips": CLIPS}, "tests/golden/color_long_window.npz was made with other parameters"
    return {k: g[k] for k in g.files}


def _b_run(lvm, lib, mem, name, stop=None):
    """clip `name` (its first `stop` frames) through lvm_process_device_frames in the calls of its segments: (produced flags, frames,
    variants of col_dft up to window length 1024, variants beyond, col_dft launches of every call of more than one frame)"""
    clip = CLIPS[name]
    n = clip["frames"] if stop is None else stop
    frames = np.stack([frame6(t) for t in range(n)])
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.profile(True)
        ctx.profile_only("col_dft")
        d_in = mem.upload(frames)
        d_out = mem.zeros_like(d_in)
        prod, batches, short = [], [], None
        for t0, cnt, per, lo, hi in clip["segments"]:
            cp = c_params(lvm, dict(BASE, framerate=clip["framerate"], coLow=lo, coHigh=hi))
            for t in range(t0, min(t0 + cnt, n), per):
                per = min(per, n - t)
                if t == SHORT_MAX:
                    short = ctx.profile_variants().get("col_dft", set())
                    ctx.profile_only("col_dft")                                     # clears what has been recorded so far
                before = _launches(ctx) if per > 1 else 0
                prod += ctx.process_device_frames(cp, per, mem.ptr(d_in, t), W, H, 1, W, W * H, W * H, mem.ptr(d_out, t), W, W * H, W * H, mem.stream())
                if per > 1:
                    batches.append(_launches(ctx) - before)
        mem.sync(ctx)
        out = np.array(mem.download(d_out), copy=True)
        return prod, out, short, ctx.profile_variants().get("col_dft", set()), batches
    finally:
        ctx.close()


def _b_check(lvm, lib, mem, name, beyond="long", stop=None):
    g, clip = _golden(), CLIPS[name]
    prod, out, short, variants, batches = _b_run(lvm, lib, mem, name, stop)
    assert prod == [bool(x) for x in g[name + "_produced"][:len(prod)]], "produced flags differ from the oracle's"
    got = out[clip["keep_from"]:]
    want = g[name + "_frames"][:len(got)]
    bad = [(clip["keep_from"] + k, int((got[k] != want[k]).sum())) for k in range(len(want)) if not np.array_equal(got[k], want[k])]
    assert not bad, "%d frames differ from the oracle's, (frame, bytes) %s" % (len(bad), bad[:8])
    assert short and short <= {"thin8-128", "thin8", "thin", "wave"}, short     # windows up to 1024 frames: their own kernels, never "long" / "serial"
    assert variants == {beyond}, variants
    return batches


def test_golden_file_is_this_oracles(po):
    """the oracle over the first 1100 frames of clip A (windows up to 1100 frames: a few seconds) gives the stored frames 1000..1099"""
    g = _golden()
    clip = CLIPS["a"]
    t0, cnt, _, lo, hi = clip["segments"][0]
    assert t0 == 0 and cnt >= 1100
    P = po.make_params(framerate=clip["framerate"], coLow=lo, coHigh=hi, **BASE)
    orc = po.Oracle()
    try:
        for t in range(1100):
            out, pr = orc.process(frame6(t), P)
            assert bool(pr) == bool(g["a_produced"][t]), t
            if t >= clip["keep_from"]:
                assert np.array_equal(out, g["a_frames"][t - clip["keep_from"]]), "frame %d" % t
    finally:
        orc.close()
    for name in CLIPS:
        assert g[name + "_frames"].shape == (CLIPS[name]["frames"] - CLIPS[name]["keep_from"], H, W)
        assert all(np.unique(f).size >= 16 for f in g[name + "_frames"])


def test_window2048_emu(lvm, emu):
    assert _b_check(lvm, emu, HOST, "a") == [1, 1]                  # the 32-frame and the 8-frame call: one col_dft launch each


def test_window4096_emu(lvm, emu):
    assert _b_check(lvm, emu, HOST, "b") == [1]


def test_window2048_serial_switch_emu(lvm, emu, monkeypatch):
    """the kernel these windows had before (LVM_COL_LONG_DFT=0) against the same file, over the window lengths 1025..1100 (its inverse
    walks all n / 2 bins for every sample whatever the band: the whole clip takes the emulation 40 s -- it gave the file's bytes too)"""
    monkeypatch.setenv("LVM_COL_LONG_DFT", "0")
    assert _b_check(lvm, emu, HOST, "a", beyond="serial", stop=1100) == []


@pytest.mark.gpu
def test_window2048_gpu(lvm, hip, dev):
    assert _b_check(lvm, hip, dev, "a") == [1, 1]


@pytest.mark.gpu
def test_window4096_gpu(lvm, hip, dev):
    assert _b_check(lvm, hip, dev, "b") == [1]
