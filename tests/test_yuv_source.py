"""Chain input in raw camera formats (lvm_set_source_format, include/lvm_hip.h): YUYV, UYVY, YVYU, NV12, NV21 frames in front of
PreprocessProcessor, converted on the device by the kernel that crops and decimates (csrc/preprocess.hip).

The definition: with format F the chain / export / preprocess surfaces give, byte for byte, what the same call gives on
cvtColor(frame, COLOR_YUV2BGR_F).  The yardstick here is a NumPy restatement of OpenCV 4's color_yuv (ITU-R BT.601, limited range, 20-bit
fixed point, chroma replicated; `to_bgr` below) whose BGR frames go through the existing oracle (po.preprocess) or through a second
context of the same library that is fed BGR frames.  The restatement is pinned by hand-computed known answers; it is UNPINNED AT THE
OPENCV BOUNDARY, as tests/test_preprocess.py is for the stages behind it: there is no OpenCV on the build box.  tools/pin_with_opencv.sh
renders cv2.cvtColor of one fixed raw frame per format into tests/golden/yuv_cvtcolor.npz where OpenCV exists; the refpin test at the end
compares with it and skips while the file is absent.

Every check runs on the CPU emulation build and, under -m gpu, on the gfx950 library, through the same _check_* helpers."""
import ctypes
import os

import numpy as np
import pytest

from helpers import HostMem, TorchMem, c_params
from test_preprocess import CASES, _frame, _params

BGR, YUYV, UYVY, YVYU, NV12, NV21 = range(6)
FORMATS = (YUYV, UYVY, YVYU, NV12, NV21)
NAMES = {YUYV: "YUYV", UYVY: "UYVY", YVYU: "YVYU", NV12: "NV12", NV21: "NV21"}
PACKED = {YUYV: (0, 1, 3), UYVY: (1, 0, 2), YVYU: (0, 3, 1)}      # byte of Y0 (Y1 two behind it), of U, of V inside a 4-byte pair
INVALID = -1                                                       # LVM_ERR_INVALID
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yuv_cvtcolor.npz")


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def yuv2bgr(Y, U, V):
    """OpenCV 4 color_yuv on int arrays of equal shape -> uint8 [..., 3] (B, G, R).  int32 as in OpenCV: test_restatement_fits_int32 shows
    that it holds every sum.  NumPy's >> on signed integers is arithmetic: negative sums floor."""
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * 1220542 + (1 << 19)
    u, v = U - 128, V - 128
    r = (y + 1673527 * v) >> 20
    g = (y - 852492 * v - 409993 * u) >> 20
    b = (y + 2116026 * u) >> 20
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def planes(raw, fmt):
    """(Y, U, V) per pixel, each [h][w], of a raw frame: chroma replicated over the pair (4:2:2) / the 2 x 2 block (NV12, NV21)"""
    if fmt in PACKED:
        yo, uo, vo = PACKED[fmt]
        h, w = raw.shape[0], raw.shape[1] // 2
        q = raw.reshape(h, w // 2, 4)
        Y = np.stack([q[:, :, yo], q[:, :, yo + 2]], axis=-1).reshape(h, w)
        return Y, np.repeat(q[:, :, uo], 2, axis=1), np.repeat(q[:, :, vo], 2, axis=1)
    h, w = raw.shape[0] // 3 * 2, raw.shape[1]
    uv = raw[h:].reshape(h // 2, w // 2, 2)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    return raw[:h], up(uv[:, :, 0 if fmt == NV12 else 1]), up(uv[:, :, 1 if fmt == NV12 else 0])


def to_bgr(raw, fmt):
    """cvtColor(raw, COLOR_YUV2BGR_<fmt>) restated"""
    return yuv2bgr(*planes(raw, fmt))


def raw_shape(fmt, w, h):
    return (h, 2 * w) if fmt in PACKED else (h * 3 // 2, w)


def raw_random(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=raw_shape(fmt, w, h), dtype=np.uint8)


def raw_from_bgr(f, fmt):
    """A raw frame with the content of a BGR frame (any fixed map will do: Y = G, U = B, V = R of the pair's / block's first pixel): clips
    with structure for the magnifier behind the conversion"""
    h, w = f.shape[:2]
    if fmt in PACKED:
        yo, uo, vo = PACKED[fmt]
        q = np.empty((h, w // 2, 4), np.uint8)
        q[:, :, yo], q[:, :, yo + 2] = f[:, 0::2, 1], f[:, 1::2, 1]
        q[:, :, uo], q[:, :, vo] = f[:, 0::2, 0], f[:, 0::2, 2]
        return q.reshape(h, 2 * w)
    raw = np.empty((h * 3 // 2, w), np.uint8)
    raw[:h] = f[:, :, 1]
    uv = raw[h:].reshape(h // 2, w // 2, 2)
    uv[:, :, 0 if fmt == NV12 else 1] = f[0::2, 0::2, 0]
    uv[:, :, 1 if fmt == NV12 else 0] = f[0::2, 0::2, 2]
    return raw


def _none(lvm):
    return lvm.LvmParams(3, 1, 0, 0, 0, 0, 0, 30.0, 0)            # mode None: the chain returns the preprocessed frame


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    """(Y, U, V) -> (B, G, R), by hand:
    (16, 128, 128): y = 0, all three sums 2^19 -> 0.   (235, 128, 128): 219 * 1220542 + 2^19 = 267822986 -> 255.4 -> 255.
    (0, 128, 128): max(0, -16) = 0 -> black.
    (81, 90, 240): y = 65 * 1220542 + 524288 = 79859518; R: + 1673527 * 112 = 267294542 -> 254 (254.9 floors);
      G: - 852492 * 112 + 409993 * 38 = -39852 -> floors to -1 -> 0;  B: - 2116026 * 38 = -549470 -> -1 -> 0.  A logical shift would give
      4095 -> 255 for both; the sums and their shifts are checked directly below."""
    got = yuv2bgr([16, 235, 0, 81], [128, 128, 128, 90], [128, 128, 128, 240])
    assert got.tolist() == [[0, 0, 0], [255, 255, 255], [0, 0, 0], [0, 0, 254]]
    y = 65 * 1220542 + (1 << 19)
    assert y - 852492 * 112 - 409993 * (90 - 128) == -39852 and y + 2116026 * (90 - 128) == -549470
    assert (-39852 >> 20) == -1 and (-549470 >> 20) == -1 and (y + 1673527 * 112) >> 20 == 254
    # pure colours of BT.601 studio range: red (81, 90, 240), green (145, 54, 34), blue (41, 240, 110) -> within 1 of the primaries
    prim = yuv2bgr([145, 41], [54, 240], [34, 110]).astype(int)
    assert np.abs(prim - np.array([[0, 255, 0], [255, 0, 0]])).max() <= 1


def test_restatement_fits_int32():
    ymax = (255 - 16) * 1220542 + (1 << 19)
    assert ymax + 2116026 * 127 < 2 ** 31 and (1 << 19) - 2116026 * 128 > -2 ** 31
    assert ymax + 852492 * 128 + 409993 * 128 < 2 ** 31 and (1 << 19) - 852492 * 127 - 409993 * 127 > -2 ** 31


def test_restatement_layouts():
    """which byte is which: one 2 x 2 frame per format, distinct values"""
    Y = np.array([[50, 60], [70, 80]])
    assert np.array_equal(to_bgr(np.array([[50, 90, 60, 200], [70, 91, 80, 201]], np.uint8), YUYV), yuv2bgr(Y, [[90, 90], [91, 91]], [[200, 200], [201, 201]]))
    assert np.array_equal(to_bgr(np.array([[90, 50, 200, 60], [91, 70, 201, 80]], np.uint8), UYVY), yuv2bgr(Y, [[90, 90], [91, 91]], [[200, 200], [201, 201]]))
    assert np.array_equal(to_bgr(np.array([[50, 200, 60, 90], [70, 201, 80, 91]], np.uint8), YVYU), yuv2bgr(Y, [[90, 90], [91, 91]], [[200, 200], [201, 201]]))
    assert np.array_equal(to_bgr(np.array([[50, 60], [70, 80], [90, 200]], np.uint8), NV12), yuv2bgr(Y, np.full((2, 2), 90), np.full((2, 2), 200)))
    assert np.array_equal(to_bgr(np.array([[50, 60], [70, 80], [200, 90]], np.uint8), NV21), yuv2bgr(Y, np.full((2, 2), 90), np.full((2, 2), 200)))
    for fmt in FORMATS:                                            # raw_from_bgr writes the layout planes() reads
        f = _frame(8, 4, 3, fmt)
        Yp, U, V = planes(raw_from_bgr(f, fmt), fmt)
        ys = 1 if fmt in PACKED else 2
        assert np.array_equal(Yp, f[:, :, 1]) and np.array_equal(U[::ys, ::2], f[::ys, ::2, 0]) and np.array_equal(V[::ys, ::2], f[::ys, ::2, 2])
        assert np.array_equal(U[:, 1::2], U[:, ::2]) and (fmt in PACKED or np.array_equal(V[1::2], V[::2]))


# ---- 1. all 2^24 (Y, U, V) once ------------------------------------------------------------------------------------------------------
_ALL = {}


def _all_yuv():
    """A 4096 x 4096 YUYV frame whose 2^23 pairs enumerate every (Y0, Y1 = 255 - Y0, U, V): pair p has Y0 = p & 127, U = (p >> 7) & 255,
    V = p >> 15 -- every (Y, U, V) exactly once.  And the restatement's BGR frame.  Computed once, shared, never written."""
    if not _ALL:
        p = np.arange(1 << 23, dtype=np.uint32)
        q = np.empty((1 << 23, 4), np.uint8)
        q[:, 0] = p & 127
        q[:, 2] = 255 - q[:, 0]
        q[:, 1] = (p >> 7) & 255
        q[:, 3] = p >> 15
        raw = q.reshape(4096, 8192)
        seen = np.zeros(1 << 24, bool)
        Y, U, V = planes(raw, YUYV)
        seen[(Y.astype(np.uint32) << 16 | U.astype(np.uint32) << 8 | V).reshape(-1)] = True
        assert seen.all()
        _ALL["raw"], _ALL["bgr"] = raw, to_bgr(raw, YUYV)
        _ALL["raw"].setflags(write=False); _ALL["bgr"].setflags(write=False)
    return _ALL["raw"], _ALL["bgr"]


def _check_all_values(lvm, lib, rows=None):
    """crop-only through lvm_chain_process: the vector kernel on whole frames ("yuv4"), then -- grayscale on, the colour frame read from the
    tap of lvm_chain_process_batch_ex -- the byte kernel ("yuv") on every 64th row.  rows: a slice of the frame's rows (None: all)."""
    raw, bgr = _all_yuv()
    if rows is not None:
        raw, bgr = raw[rows], bgr[rows]
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.set_source_format(YUYV)
        ctx.profile(True)
        out, produced = ctx.chain_process(raw, lvm.to_c_preprocess(lvm.PreprocessParams(), False), _none(lvm))
        assert not produced and out.shape == bgr.shape
        bad = np.flatnonzero((out != bgr).any(axis=2).reshape(-1))
        assert bad.size == 0, "%d pixels differ, first at pair %d: got %s, want %s" % (bad.size, bad[0] // 2, out.reshape(-1, 3)[bad[0]], bgr.reshape(-1, 3)[bad[0]])
        assert ctx.profile_variants()["preprocess"] == {"yuv4"}
        ctx.profile_only("preprocess")
        sl = np.ascontiguousarray(raw[::64])
        _, taps, _ = ctx.chain_process_batch_ex([sl], lvm.to_c_preprocess(lvm.PreprocessParams(), True), _none(lvm))
        assert np.array_equal(taps[0], bgr[::64])
        assert ctx.profile_variants()["preprocess"] == {"yuv"}
    finally:
        ctx.close()


def test_all_yuv_values_emu(lvm, emu):
    _check_all_values(lvm, emu)


@pytest.mark.gpu
def test_all_yuv_values_gpu(lvm, hip):
    _check_all_values(lvm, hip)


# ---- 2. formats x geometry -----------------------------------------------------------------------------------------------------------
GEOMETRY = [  # (w, h, downscale, roi, grayscale)
    (64, 48, 1, None, False),                                  # crop-only at full size: the plain conversion (vector kernel)
    (64, 48, 2, None, False),                                  # 2 x 2 blocks of converted bytes: (sum + 2) >> 2
    (70, 46, 4, (0.1, 0.1, 0.8, 0.8), False),                  # ROI (7, 5) 56 x 37 -> 14 x 9: fractional rows (area tables), odd origin
    (64, 48, 1, (11 / 64, 7 / 48, 0.5, 0.5), True),            # ROI at odd x AND odd y: pair / block parity; gray + the colour tap
    (64, 48, 2, (11 / 64, 7 / 48, 0.5, 0.5), True),            # the same, decimated
    (64, 48, 8, (0.52, 0.52, 0.05, 0.05), False),              # ROI (33, 25) 3 x 2, smaller than the divisor: 1 x 1 output
    (66, 48, 1, None, False),                                  # even width, no multiple of 4: the vector kernel does not apply
    (64, 48, 1, (0.125, 0.25, 0.5, 0.5), False),               # ROI at even x, even y, width 32: crop-only on the vector kernel
    (64, 48, 1, (6 / 64, 0.25, 0.5, 0.5), False),              # ROI at x = 6: a pair boundary that is no dword of Y (NV12)
    (64, 48, 3, (0.9, 0.9, 0.5, 0.5), True),                   # clipped at the frame edge, divisor 3
]


def _check_geometry(lvm, po, lib, fmt):
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.set_source_format(fmt)
        assert ctx.source_format() == fmt
        for i, (w, h, ds, roi, gray) in enumerate(GEOMETRY):
            raw = raw_random(fmt, w, h, 1000 * fmt + i)
            bgr = to_bgr(raw, fmt)
            cpre, opre = _params(lvm, po, ds, roi, gray)
            _, opre_tap = _params(lvm, po, ds, roi, False)
            want, want_tap = po.preprocess(bgr, opre), po.preprocess(bgr, opre_tap)
            assert ctx.preprocess_geometry(cpre, w, h, 3) == po.preprocess_geometry(opre, w, h, 3)
            out, produced = ctx.chain_process(raw, cpre, _none(lvm))
            assert not produced
            assert out.shape == want.shape and np.array_equal(out, want), (NAMES[fmt], i, int((out != want).sum()))
            outs, taps, _ = ctx.chain_process_batch_ex([raw], cpre, _none(lvm))
            assert np.array_equal(outs[0], want), (NAMES[fmt], i)
            assert taps[0].shape == want_tap.shape and np.array_equal(taps[0], want_tap), (NAMES[fmt], i, "tap")
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_formats_geometry_emu(lvm, po, emu, fmt):
    _check_geometry(lvm, po, emu, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_formats_geometry_gpu(lvm, po, hip, fmt):
    _check_geometry(lvm, po, hip, fmt)


# layouts of lvm_preprocess_device: (input row padding, input base offset, output row padding, output base offset) -> the variant that must run
LAYOUTS = [((0, 0, 0, 0), "yuv4"), ((8, 0, 4, 0), "yuv4"), ((4, 4, 0, 8), "yuv4"), ((3, 0, 0, 0), "yuv"), ((0, 1, 0, 0), "yuv"), ((0, 2, 0, 0), "yuv"),
           ((0, 0, 1, 0), "yuv"), ((0, 0, 0, 2), "yuv")]


def _check_device_layouts(lvm, po, lib, mem, fmt):
    """lvm_preprocess_device on two streams of device-resident raw frames, crop-only, under padded strides and offset base pointers: the
    variant the layout calls for ran (lvm_profile_variants), all layouts give the restatement's bytes -- so the two variants give identical
    bytes -- and nothing outside the output rows is written.  Then one decimating call on the same frames (always the byte kernel)."""
    w, h, S = 64, 48, 2
    raws = [raw_random(fmt, w, h, 50 * fmt + s) for s in range(S)]
    want = [to_bgr(r, fmt) for r in raws]
    rh, rb = raws[0].shape
    cpre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
    ctx = lvm.Context(0, S, lib)
    try:
        ctx.set_source_format(fmt)
        ctx.profile(True)
        for (pi, oi, po_, oo), variant in LAYOUTS:
            si, so = rb + pi, w * 3 + po_
            fin, fout = rh * si + 16, h * so + 16                   # one stream's allocation: the rows, and room for the base offset
            buf = np.full(S * fin, 0xAB, np.uint8)
            for s in range(S):
                v = buf[s * fin + oi: s * fin + oi + rh * si].reshape(rh, si)
                v[:, :rb] = raws[s]
            d_in, d_out = mem.upload(buf), mem.upload(np.full(S * fout, 0xCD, np.uint8))
            assert mem.ptr_at(d_in, 0) % 16 == 0 and mem.ptr_at(d_out, 0) % 16 == 0
            ctx.profile_only("preprocess")
            ctx.preprocess_device(cpre, ctypes.c_void_p(mem.ptr_at(d_in, oi)), w, h, 3, si, fin, ctypes.c_void_p(mem.ptr_at(d_out, oo)), so, fout, mem.stream())
            mem.sync(ctx)
            assert ctx.profile_variants()["preprocess"] == {variant}, ((pi, oi, po_, oo), ctx.profile_variants())
            got = mem.download(d_out)
            touched = np.zeros(S * fout, bool)
            for s in range(S):
                idx = s * fout + oo + np.arange(h)[:, None] * so + np.arange(w * 3)[None, :]
                touched[idx.reshape(-1)] = True
                assert np.array_equal(got[idx].reshape(h, w, 3), want[s]), (NAMES[fmt], (pi, oi, po_, oo), s)
            assert (got[~touched] == 0xCD).all(), "bytes outside the output rows were written"
        cpre2, opre2 = _params(lvm, po, 2, (3 / 64, 5 / 48, 0.75, 0.75), True)
        _, _, _, _, ow, oh, och = ctx.preprocess_geometry(cpre2, w, h, 3)
        d_in = mem.upload(np.stack(raws))
        d_out = mem.upload(np.zeros((S, oh, ow), np.uint8))
        ctx.preprocess_device(cpre2, ctypes.c_void_p(mem.ptr(d_in)), w, h, 3, rb, rh * rb, ctypes.c_void_p(mem.ptr(d_out)), ow, ow * oh, mem.stream())
        mem.sync(ctx)
        got = mem.download(d_out)
        for s in range(S):
            assert np.array_equal(got[s], po.preprocess(want[s], opre2)), (NAMES[fmt], s)
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_device_layouts_emu(lvm, po, emu, fmt):
    _check_device_layouts(lvm, po, emu, HostMem(), fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_device_layouts_gpu(lvm, po, hip, fmt):
    _check_device_layouts(lvm, po, hip, TorchMem(), fmt)


# ---- 3. streams ------------------------------------------------------------------------------------------------------------------------
def _clips(lvm, fmt, n_streams, nframes, size=(96, 64, 3), cfg=0):
    """per stream: raw frames with the content of a synthetic clip, and the BGR frames they convert to"""
    ck, pk = lvm.synth.config(cfg, size)
    clips = [lvm.synth.Clip(seed=77 + s, **ck) for s in range(n_streams)]
    raws = [[raw_from_bgr(c.frame(t), fmt) for c in clips] for t in range(nframes)]
    return raws, [[to_bgr(r, fmt) for r in row] for row in raws], pk


def _check_streams(lvm, po, lib, fmt, exact):
    raws, bgrs, pk = _clips(lvm, fmt, 3, 6)
    cpre, _ = _params(lvm, po, 2, (0.05, 0.1, 0.9, 0.8), False)
    a, b = lvm.Context(0, 3, lib), lvm.Context(0, 3, lib)
    try:
        a.exact_lab(exact); b.exact_lab(exact)
        a.set_source_format(fmt)
        flags = []
        for t in range(6):
            oa, pa = a.chain_process_batch(raws[t], cpre, c_params(lvm, pk))
            ob, pb = b.chain_process_batch(bgrs[t], cpre, c_params(lvm, pk))
            assert pa == pb, t
            flags.append(pa)
            for s in range(3):
                assert np.array_equal(oa[s], ob[s]), (NAMES[fmt], t, s, int((oa[s] != ob[s]).sum()))
        assert any(flags)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("fmt", (NV12, YUYV), ids=("NV12", "YUYV"))
def test_streams_emu(lvm, po, emu, fmt):
    _check_streams(lvm, po, emu, fmt, True)
    _check_streams(lvm, po, emu, fmt, False)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", (NV12, YUYV), ids=("NV12", "YUYV"))
def test_streams_gpu(lvm, po, hip, fmt):
    _check_streams(lvm, po, hip, fmt, True)
    _check_streams(lvm, po, hip, fmt, False)


# ---- 4. the other surfaces ---------------------------------------------------------------------------------------------------------------
def _check_present(lvm, po, lib, alloc, fmt):
    raws, bgrs, pk = _clips(lvm, fmt, 1, 4)
    cpre, _ = _params(lvm, po, 2, (5 / 96, 3 / 64, 0.8, 0.8), True)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        a.set_source_format(fmt)
        _, _, _, _, ow, oh, och = a.preprocess_geometry(cpre, 96, 64, 3)
        for t in range(4):
            res = []
            for ctx, f in ((a, raws[t][0]), (b, bgrs[t][0])):
                dp, read_p = alloc(oh * ow * och)
                do, read_o = alloc(oh * ow * 3)
                pr = ctx.chain_present(f, cpre, c_params(lvm, pk), dp, ow * och, do, ow * 3)
                res.append((pr, read_p(), read_o()))
            assert res[0][0] == res[1][0], t
            assert np.array_equal(res[0][1], res[1][1]), (t, "processed pane")
            assert np.array_equal(res[0][2], res[1][2]), (t, "original pane")
    finally:
        a.close(); b.close()


def _check_export(lvm, po, lib, fmt):
    """split left-right over 20 frames: ten sub-batches of the three-queue pipeline; then the same frames to JPEG"""
    raws, bgrs, pk = _clips(lvm, fmt, 1, 20)
    cpre, _ = _params(lvm, po, 1, (7 / 96, 5 / 64, 0.75, 0.75), False)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        a.set_source_format(fmt)
        ca, pa = a.export_frames([r[0] for r in raws], cpre, c_params(lvm, pk), 1)
        cb, pb = b.export_frames([r[0] for r in bgrs], cpre, c_params(lvm, pk), 1)
        assert pa == pb and any(pa)
        for t in range(20):
            assert np.array_equal(ca[t], cb[t]), (NAMES[fmt], t)
        a.reset(); b.reset()
        assert a.source_format() == fmt                            # lvm_reset keeps the format
        ja, pa = a.export_frames_mjpeg([r[0] for r in raws[:6]], cpre, c_params(lvm, pk), 1, 80)
        jb, pb = b.export_frames_mjpeg([r[0] for r in bgrs[:6]], cpre, c_params(lvm, pk), 1, 80)
        assert pa == pb and ja == jb
    finally:
        a.close(); b.close()


def _alloc_host(keep):
    def alloc(n):
        buf = np.full(n, 0x5A, np.uint8)
        keep.append(buf)
        return buf.ctypes.data, (lambda: buf.copy())
    return alloc


def _alloc_gpu():
    import torch

    def alloc(n):
        t = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t.data_ptr(), (lambda: t.cpu().numpy())
    return alloc


@pytest.mark.parametrize("fmt", (UYVY, NV21), ids=("UYVY", "NV21"))
def test_present_emu(lvm, po, emu, fmt):
    _check_present(lvm, po, emu, _alloc_host([]), fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", (UYVY, NV21), ids=("UYVY", "NV21"))
def test_present_gpu(lvm, po, hip, fmt):
    _check_present(lvm, po, hip, _alloc_gpu(), fmt)


@pytest.mark.parametrize("fmt", (YUYV, NV12), ids=("YUYV", "NV12"))
def test_export_emu(lvm, po, emu, fmt):
    _check_export(lvm, po, emu, fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", (YUYV, NV12), ids=("YUYV", "NV12"))
def test_export_gpu(lvm, po, hip, fmt):
    _check_export(lvm, po, hip, fmt)


# ---- 5. off by default, refusals -----------------------------------------------------------------------------------------------------
def _check_default_and_back(lvm, po, lib):
    ctx = lvm.Context(0, 1, lib)
    try:
        assert ctx.source_format() == BGR
        ctx.set_source_format(YUYV)
        ctx.set_source_format(BGR)
        assert ctx.source_format() == BGR
        for i in (4, 2, 9):                                         # ROI + fractional cells + gray; a gray source; the identity
            w, h, ch, ds, roi, gray = CASES[i]
            f = _frame(w, h, ch, 100 + i)
            cpre, opre = _params(lvm, po, ds, roi, gray)
            out, produced = ctx.chain_process(f, cpre, _none(lvm))
            assert not produced and np.array_equal(out, po.preprocess(f, opre)), i
    finally:
        ctx.close()


def _check_refusals(lvm, po, lib):
    """a context that is refused five ways in the middle of a clip against an undisturbed twin: every refusal is LVM_ERR_INVALID with a
    message that names the rule, and the clip goes on as if nothing had happened"""
    raws, _, pk = _clips(lvm, YUYV, 1, 8)
    nv = [raw_from_bgr(lvm.synth.Clip(seed=77, **lvm.synth.config(0, (96, 64, 3))[0]).frame(t), NV12) for t in range(8)]
    cpre = lvm.to_c_preprocess(lvm.PreprocessParams(), False)
    cp = c_params(lvm, pk)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    out = np.zeros((64, 96, 3), np.uint8)
    produced = ctypes.c_int(7)

    def refused(w, h, ch, stride, frame, match):
        rc = lib.lvm_chain_process(a.h, ctypes.byref(cpre), ctypes.byref(cp), frame.ctypes.data, w, h, ch, stride, out.ctypes.data, 96 * 3, ctypes.byref(produced))
        assert rc == INVALID and produced.value == 0
        assert match in lib.lvm_last_error(a.h).decode(), lib.lvm_last_error(a.h).decode()

    try:
        for ctx in (a, b):
            ctx.set_source_format(YUYV)
        for t in range(8):
            if t == 4:
                refused(95, 64, 3, 192, raws[t][0], "w must be even")
                refused(96, 64, 1, 192, raws[t][0], "channels must be 3")
                refused(96, 64, 3, 191, raws[t][0], "in_stride must be >= 2 * w")
                a.set_source_format(NV12)
                refused(96, 63, 3, 96, nv[t], "h must be even")
                refused(96, 64, 3, 95, nv[t], "in_stride must be >= w")
                assert lib.lvm_set_source_format(a.h, 6) == INVALID and lib.lvm_set_source_format(a.h, -1) == INVALID
                assert "lvm_set_source_format" in lib.lvm_last_error(a.h).decode()
                assert a.source_format() == NV12                   # an unknown format changes nothing
                a.set_source_format(YUYV)
            oa, pa = a.chain_process(raws[t][0], cpre, cp)
            ob, pb = b.chain_process(raws[t][0], cpre, cp)
            assert pa == pb and (pa or t == 0), t
            assert np.array_equal(oa, ob), t
    finally:
        a.close(); b.close()


def test_default_and_back_emu(lvm, po, emu):
    _check_default_and_back(lvm, po, emu)


def test_refusals_emu(lvm, po, emu):
    _check_refusals(lvm, po, emu)


@pytest.mark.gpu
def test_default_and_refusals_gpu(lvm, po, hip):
    _check_default_and_back(lvm, po, hip)
    _check_refusals(lvm, po, hip)


# ---- 6. format switch in the middle of a clip -----------------------------------------------------------------------------------------
def _check_switch(lvm, po, lib, exact):
    """four frames as BGR, then the same scene as YUYV, against an all-BGR context: the setter does not disturb the temporal state"""
    raws, bgrs, pk = _clips(lvm, YUYV, 1, 10)
    cpre, _ = _params(lvm, po, 2, None, False)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        a.exact_lab(exact); b.exact_lab(exact)
        for t in range(10):
            if t == 4:
                a.set_source_format(YUYV)
            oa, pa = a.chain_process(raws[t][0] if t >= 4 else bgrs[t][0], cpre, c_params(lvm, pk))
            ob, pb = b.chain_process(bgrs[t][0], cpre, c_params(lvm, pk))
            assert pa == pb and (pa or t == 0), t                   # (a structural reset at the switch would show as produced = False)
            assert np.array_equal(oa, ob), t
    finally:
        a.close(); b.close()


def test_format_switch_emu(lvm, po, emu):
    _check_switch(lvm, po, emu, True)


@pytest.mark.gpu
def test_format_switch_gpu(lvm, po, hip):
    _check_switch(lvm, po, hip, True)
    _check_switch(lvm, po, hip, False)


# ---- the OpenCV boundary -----------------------------------------------------------------------------------------------------------------
def golden_raw(fmt):
    """the fixed raw frame of tools/pin_with_opencv.sh: 32 x 16, seed 9000 + format"""
    return raw_random(fmt, 32, 16, 9000 + fmt)


@pytest.mark.refpin
def test_restatement_against_opencv_golden():
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/yuv_cvtcolor.npz is absent: run tools/pin_with_opencv.sh where OpenCV 4 is installed")
    gold = np.load(GOLDEN)
    for fmt in FORMATS:
        assert np.array_equal(gold["raw_" + NAMES[fmt]], golden_raw(fmt))
        assert np.array_equal(gold["bgr_" + NAMES[fmt]], to_bgr(golden_raw(fmt), fmt)), NAMES[fmt]
