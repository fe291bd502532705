"""Export canvases as 4:2:0 surfaces (lvm_set_canvas_format, include/lvm_hip.h): NV12 / NV21 / I420 / YV12 canvases out of lvm_export_frames and
lvm_canvas_convert_device, converted on the device by k_canvas_yuv (csrc/compose.hip).

The definition: with canvas format F a participating surface gives cvtColor(canvas, COLOR_BGR2YUV_I420) of the BGR canvas it gives under
LVM_PIX_BGR, byte for byte, in the layout of F, the text overlay applied first.  The yardstick is a NumPy restatement of OpenCV 4's color_yuv
(ITU-R BT.601, limited range, 20-bit fixed point, chroma of the top-left pixel of each 2 x 2 block; `bgr2yuv420` below) applied to the BGR
canvases a second context of the same library gives on the same frames.  The restatement is pinned by hand-computed known answers; it is
UNPINNED AT THE OPENCV BOUNDARY, as tests/test_yuv_source.py is for the other direction: there is no OpenCV on the build box.
tools/pin_with_opencv.sh renders cv2.cvtColor(frame, COLOR_BGR2YUV_I420 / _YV12) of one fixed BGR frame into tests/golden/bgr2yuv_420.npz where
OpenCV exists; the refpin test at the end compares with it and skips while the file is absent.

Every check runs on the CPU emulation build and, under -m gpu, on the gfx950 library, through the same _check_* helpers."""
import ctypes
import os

import numpy as np
import pytest

from helpers import HostMem, TorchMem, c_params
from test_preprocess import _frame, _params
from test_yuv_source import raw_from_bgr, to_bgr

BGR, NV12, NV21, I420, YV12 = 0, 4, 5, 6, 7
FORMATS = (NV12, NV21, I420, YV12)
NAMES = {NV12: "NV12", NV21: "NV21", I420: "I420", YV12: "YV12"}
NONE, LR, TB = 0, 1, 2
INVALID = -1                                                       # LVM_ERR_INVALID
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgr2yuv_420.npz")


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def yuv_of(b, g, r):
    """OpenCV 4 color_yuv, BGR -> (Y, U, V) on int arrays of equal shape.  int32 as in OpenCV: test_restatement_fits_int32 shows that it holds
    every sum, that every sum is positive (the shift never sees a sign) and that every result is a byte (no saturation)."""
    b, g, r = (np.asarray(a).astype(np.int32) for a in (b, g, r))
    y = (269484 * r + 528482 * g + 102760 * b + (1 << 19) + (16 << 20)) >> 20
    u = (-155188 * r - 305135 * g + 460324 * b + (1 << 19) + (128 << 20)) >> 20
    v = (460324 * r - 385875 * g - 74448 * b + (1 << 19) + (128 << 20)) >> 20
    return y, u, v


def planes420(frame):
    """(Y [h][w], U [h/2][w/2], V [h/2][w/2]) of a BGR frame with even sizes: chroma of the top-left pixel of each 2 x 2 block"""
    assert frame.ndim == 3 and frame.shape[2] == 3 and frame.shape[0] % 2 == 0 and frame.shape[1] % 2 == 0
    y, _, _ = yuv_of(frame[:, :, 0], frame[:, :, 1], frame[:, :, 2])
    s = frame[0::2, 0::2]
    _, u, v = yuv_of(s[:, :, 0], s[:, :, 1], s[:, :, 2])
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def layout(fmt, w, h, stride):
    """(bytes, plane1_offset, plane2_offset, chroma_stride) by the definitions of include/lvm_hip.h"""
    if fmt == BGR:
        return stride * h, 0, 0, 0
    if fmt in (NV12, NV21):
        return stride * h * 3 // 2, stride * h, 0, stride
    return stride * h * 3 // 2, stride * h, stride * h * 5 // 4, stride // 2


def scatter(fmt, Y, U, V, stride=None, fill=0):
    """the planes into one flat buffer of `bytes` bytes in the layout of fmt, Y row stride `stride`; every other byte is `fill`"""
    h, w = Y.shape
    stride = w if stride is None else stride
    nbytes, p1, p2, cs = layout(fmt, w, h, stride)
    out = np.full(nbytes, fill, np.uint8)
    yi = np.arange(h)[:, None] * stride + np.arange(w)[None, :]
    out[yi] = Y
    if fmt in (NV12, NV21):
        ci = p1 + np.arange(h // 2)[:, None] * cs + 2 * np.arange(w // 2)[None, :]
        out[ci + (0 if fmt == NV12 else 1)] = U
        out[ci + (1 if fmt == NV12 else 0)] = V
    else:
        ci = np.arange(h // 2)[:, None] * cs + np.arange(w // 2)[None, :]
        out[ci + (p1 if fmt == I420 else p2)] = U
        out[ci + (p2 if fmt == I420 else p1)] = V
    return out


def bgr2yuv420(frame, fmt, stride=None, fill=0):
    """cvtColor(frame, COLOR_BGR2YUV_I420) restated, in the layout of fmt: a flat buffer; with stride == w (the default) it reshapes to
    OpenCV's (3h/2, w) single-channel Mat"""
    return scatter(fmt, *planes420(frame), stride=stride, fill=fill)


def as_mat(frame, fmt):
    return bgr2yuv420(frame, fmt).reshape(frame.shape[0] * 3 // 2, frame.shape[1])


# ---- 1. the restatement itself -------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    """(B, G, R) -> (Y, U, V), by hand (2^20 = 1048576; the rounding term 2^19 and the offsets 16 << 20 = 16777216, 128 << 20 = 134217728):
    black: the offsets alone -> (16, 128, 128).
    white: Y = 900726 * 255 + 524288 + 16777216 = 246986634 -> 235.54 -> 235; U = V = 1 * 255 + 524288 + 134217728 -> 128.5002 -> 128 (the
      U and V rows each sum to 1, OpenCV's quirk).
    red:   Y = 269484 * 255 + 17301504 = 86019924 -> 82.03; U = -155188 * 255 + 134742016 = 95169076 -> 90.76; V = 460324 * 255 + 134742016 =
      252124636 -> 240.44.
    green: Y = 528482 * 255 + 17301504 = 152064414 -> 145.02; U = -305135 * 255 + 134742016 = 56932591 -> 54.29; V = -385875 * 255 + 134742016 =
      36343891 -> 34.66.
    blue:  Y = 102760 * 255 + 17301504 = 43505304 -> 41.49; U = 252124636 -> 240.44; V = -74448 * 255 + 134742016 = 115757776 -> 110.39."""
    bgr = np.array([(0, 0, 0), (255, 255, 255), (0, 0, 255), (0, 255, 0), (255, 0, 0)])
    y, u, v = yuv_of(bgr[:, 0], bgr[:, 1], bgr[:, 2])
    assert np.stack([y, u, v], axis=1).tolist() == [[16, 128, 128], [235, 128, 128], [82, 90, 240], [145, 54, 34], [41, 240, 110]]
    assert 269484 * 255 + 17301504 == 86019924 and -155188 * 255 + 134742016 == 95169076 and 460324 * 255 + 134742016 == 252124636
    assert 86019924 >> 20 == 82 and 95169076 >> 20 == 90 and 252124636 >> 20 == 240
    assert -155188 - 305135 + 460324 == 1 and 460324 - 385875 - 74448 == 1 and 269484 + 528482 + 102760 == 900726


def test_restatement_fits_int32():
    """the extreme sums: each is linear in (B, G, R), so its extremes lie at corners of the cube -- positive coefficients at 255 for the maximum,
    negative ones for the minimum.  All positive and below 2^31: `>>` never sees a sign; all results in 0..255: no saturation."""
    rnd, yo, co = 1 << 19, 16 << 20, 128 << 20
    ymin, ymax = rnd + yo, 900726 * 255 + rnd + yo
    umin, umax = -(155188 + 305135) * 255 + rnd + co, 460324 * 255 + rnd + co
    vmin, vmax = -(385875 + 74448) * 255 + rnd + co, 460324 * 255 + rnd + co
    for lo, hi in ((ymin, ymax), (umin, umax), (vmin, vmax)):
        assert 0 < lo <= hi < 2 ** 31
        assert 0 <= lo >> 20 <= hi >> 20 <= 255
    assert (ymin >> 20, ymax >> 20, umin >> 20, umax >> 20, vmin >> 20, vmax >> 20) == (16, 235, 16, 240, 16, 240)
    c = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)])
    y, u, v = (x.astype(np.int64) for x in yuv_of(c[:, 0], c[:, 1], c[:, 2]))
    assert (y.min(), y.max(), u.min(), u.max(), v.min(), v.max()) == (16, 235, 16, 240, 16, 240)


def test_restatement_layouts():
    """which byte lands where: a 4 x 2 frame with distinct values per format, an I420 stride larger than w, and h / 2 odd (h = 6)"""
    f = np.array([[(200, 20, 30), (40, 250, 60), (70, 80, 190), (0, 110, 255)], [(130, 14, 150), (160, 170, 18), (255, 200, 21), (22, 230, 240)]], np.uint8)
    px = lambda y, x: [int(t) for t in yuv_of(*[int(c) for c in f[y, x]])]
    Y = [[px(y, x)[0] for x in range(4)] for y in range(2)]
    (_, U0, V0), (_, U1, V1) = px(0, 0), px(0, 2)
    assert len({U0, U1, V0, V1}) == 4 and len(set(Y[0] + Y[1])) == 8
    X = 7                                                          # the fill of bytes no plane owns
    assert bgr2yuv420(f, NV12).tolist() == Y[0] + Y[1] + [U0, V0, U1, V1]
    assert bgr2yuv420(f, NV21).tolist() == Y[0] + Y[1] + [V0, U0, V1, U1]
    assert bgr2yuv420(f, I420).tolist() == Y[0] + Y[1] + [U0, U1] + [V0, V1]
    assert bgr2yuv420(f, YV12).tolist() == Y[0] + Y[1] + [V0, V1] + [U0, U1]
    assert as_mat(f, I420).shape == (3, 4)
    # stride 6: Y rows at 0 and 6, U at 6 * 2 = 12 with row stride 3, V at 6 * 2 * 5 / 4 = 15; 18 bytes
    assert layout(I420, 4, 2, 6) == (18, 12, 15, 3)
    assert bgr2yuv420(f, I420, 6, X).tolist() == Y[0] + [X, X] + Y[1] + [X, X] + [U0, U1, X] + [V0, V1, X]
    assert bgr2yuv420(f, NV21, 5, X).tolist() == Y[0] + [X] + Y[1] + [X] + [V0, U0, V1, U1, X]
    # h = 6: three chroma rows; the second plane starts at stride * h * 5 / 4 = 30, not at a whole Y-stride row of chroma pairs
    g = np.concatenate([f, f[::-1], f], axis=0)
    assert layout(I420, 4, 6, 4) == (36, 24, 30, 2) and layout(NV12, 4, 6, 4) == (36, 24, 0, 4)
    Ug, Vg = [U0, U1, px(1, 0)[1], px(1, 2)[1], U0, U1], [V0, V1, px(1, 0)[2], px(1, 2)[2], V0, V1]
    got = bgr2yuv420(g, YV12).tolist()
    assert got[24:30] == Vg and got[30:36] == Ug and got[:8] == Y[0] + Y[1] and got[8:16] == Y[1] + Y[0]


# ---- 2. every colour once, through lvm_canvas_convert_device ---------------------------------------------------------------------------
_ALL = {}
ROLLS = ((0, 0), (0, 1), (1, 0), (1, 1))


def _all_colours():
    """A 4096 x 4096 BGR frame enumerating all 2^24 colours (pixel p: B = p & 255, G = (p >> 8) & 255, R = p >> 16), and Y, U, V of EVERY pixel.
    Chroma is sampled at even / even positions only: the frame rolled by (0, 0), (0, 1), (1, 0), (1, 1) pixels puts every colour at a sampling
    position exactly once (a roll of an even-sized frame keeps parities apart).  Computed once, shared, never written."""
    if not _ALL:
        p = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
        f = np.stack([p & 255, (p >> 8) & 255, p >> 16], axis=-1).astype(np.uint8)
        y, u, v = (a.astype(np.uint8) for a in yuv_of(f[:, :, 0], f[:, :, 1], f[:, :, 2]))
        seen = np.zeros(1 << 24, np.uint8)
        for dy, dx in ROLLS:
            seen[np.roll(p, (dy, dx), axis=(0, 1))[0::2, 0::2].reshape(-1)] += 1
        assert (seen == 1).all()
        for k, a in (("bgr", f), ("y", y), ("u", u), ("v", v)):
            a.setflags(write=False)
            _ALL[k] = a
    return _ALL["bgr"], _ALL["y"], _ALL["u"], _ALL["v"]


def _check_all_colours(lvm, lib, mem, fmts, rows=None):
    """one call with n_frames = 4 converts the four rolled frames.  rows: the even rows that start the row pairs to keep (None: all)"""
    f, y, u, v = _all_colours()
    idx = slice(None) if rows is None else np.stack([rows, rows + 1], axis=1).reshape(-1)
    frames, want = [], {fmt: [] for fmt in fmts}
    for dy, dx in ROLLS:
        r = lambda a: np.roll(a, (dy, dx), axis=(0, 1))[idx]
        frames.append(r(f))
        Y, U, V = r(y), r(u)[0::2, 0::2], r(v)[0::2, 0::2]
        for fmt in fmts:
            want[fmt].append(scatter(fmt, Y, U, V))
    h, w = frames[0].shape[:2]
    d_in = mem.upload(np.stack(frames).reshape(-1))
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.profile(True)
        for fmt in fmts:
            nbytes = layout(fmt, w, h, w)[0]
            assert ctx.canvas_layout(fmt, w, h, w)[0] == nbytes
            d_out = mem.upload(np.full(4 * nbytes, 0xCD, np.uint8))
            ctx.canvas_convert_device(fmt, ctypes.c_void_p(mem.ptr_at(d_in, 0)), w, h, w * 3, w * h * 3, 4, ctypes.c_void_p(mem.ptr_at(d_out, 0)), w, nbytes, mem.stream())
            mem.sync(ctx)
            got = mem.download(d_out).reshape(4, nbytes)
            for k in range(4):
                bad = np.flatnonzero(got[k] != want[fmt][k])
                assert bad.size == 0, "%s, roll %s: %d bytes differ, first at %d: got %d, want %d" % (NAMES[fmt], ROLLS[k], bad.size, bad[0], got[k][bad[0]], want[fmt][k][bad[0]])
        assert ctx.profile_variants()["canvas_yuv"] == {"vec8"}
    finally:
        ctx.close()


def test_all_colours_emu(lvm, emu):
    rows = np.sort(np.random.default_rng(420).choice(2048, size=24, replace=False)) * 2
    _check_all_colours(lvm, emu, HostMem(), (NV12, I420), rows)


@pytest.mark.gpu
def test_all_colours_gpu(lvm, hip):
    _check_all_colours(lvm, hip, TorchMem(), (NV12, I420))


# ---- 3. shapes and layouts against the restatement -------------------------------------------------------------------------------------
SIZES = [(2, 2), (6, 2), (8, 2), (10, 4), (24, 6), (40, 18)]      # one block of 2; the tail alone; one vector block; block + tail; h / 2 odd; several
# (input base offset, BGR row padding, output base offset, Y row padding, gap between output frames); odd Y strides are NV12 / NV21's alone
LAYOUTS = [(0, 0, 0, 0, 8), (1, 0, 0, 0, 8), (0, 0, 1, 0, 8), (0, 0, 0, 2, 8), (0, 0, 0, 4, 8), (0, 0, 0, 8, 8), (0, 2, 0, 0, 8), (0, 4, 4, 0, 0), (0, 0, 0, 0, 6), (0, 0, 0, 1, 8), (1, 1, 3, 3, 5)]


def want_vec8(fmt, w, h, in_ptr, bgr_stride, bgr_fs, out_ptr, stride, out_fs):
    """include/lvm_hip.h: dword-wide loads and stores when every pointer, stride and plane offset involved is dword-aligned and w % 8 == 0"""
    _, p1, p2, cs = layout(fmt, w, h, stride)
    return w % 8 == 0 and all(v % 4 == 0 for v in (in_ptr, bgr_stride, bgr_fs, out_ptr, stride, out_fs, p1, p2, cs))


def _check_shapes(lvm, lib, mem, fmt):
    n = 3
    ctx = lvm.Context(0, 1, lib)
    seen = set()
    try:
        ctx.profile(True)
        for si, (w, h) in enumerate(SIZES):
            frames = [_frame(w, h, 3, 7000 + 10 * si + k) for k in range(n)]
            for (ioff, ipad, ooff, opad, gap) in LAYOUTS:
                stride = w + opad
                if stride % 2 and fmt in (I420, YV12):
                    continue
                bstride = w * 3 + ipad
                bfs = bstride * h + 4
                nbytes, p1, p2, cs = layout(fmt, w, h, stride)
                assert ctx.canvas_layout(fmt, w, h, stride) == (nbytes, p1, p2, cs)
                ofs = nbytes + gap
                src = np.full(n * bfs + 16, 0xAB, np.uint8)
                want = np.full(n * ofs + 16, 0xCD, np.uint8)
                for k in range(n):
                    rows = src[ioff + k * bfs: ioff + k * bfs + h * bstride].reshape(h, bstride)
                    rows[:, :w * 3] = frames[k].reshape(h, w * 3)
                    # (0xCD in every byte no plane owns: row padding, the gaps between planes and frames)
                    want[ooff + k * ofs: ooff + k * ofs + nbytes] = bgr2yuv420(frames[k], fmt, stride, 0xCD)
                d_in, d_out = mem.upload(src), mem.upload(np.full(n * ofs + 16, 0xCD, np.uint8))
                pi, po_ = mem.ptr_at(d_in, ioff), mem.ptr_at(d_out, ooff)
                assert (pi - ioff) % 16 == 0 and (po_ - ooff) % 16 == 0
                ctx.profile_only("canvas_yuv")
                ctx.canvas_convert_device(fmt, ctypes.c_void_p(pi), w, h, bstride, bfs, n, ctypes.c_void_p(po_), stride, ofs, mem.stream())
                mem.sync(ctx)
                got = mem.download(d_out)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (NAMES[fmt], (w, h), (ioff, ipad, ooff, opad, gap), "first differing byte %d: got %d, want %d" % (bad[0], got[bad[0]], want[bad[0]]))
                variant = "vec8" if want_vec8(fmt, w, h, pi, bstride, bfs, po_, stride, ofs) else "bytes"
                assert ctx.profile_variants()["canvas_yuv"] == {variant}, (NAMES[fmt], (w, h), (ioff, ipad, ooff, opad, gap), ctx.profile_variants())
                seen.add(variant)
        assert seen == {"vec8", "bytes"}
    finally:
        ctx.close()


def test_layout_function(lvm, emu):
    """lvm_canvas_layout against the definitions, and its refusals"""
    ctx = lvm.Context(0, 1, emu)
    try:
        assert ctx.canvas_layout(BGR, 10, 4, 32) == (128, 0, 0, 0)
        assert ctx.canvas_layout(NV12, 10, 4, 11) == (66, 44, 0, 11) and ctx.canvas_layout(NV21, 10, 4, 10) == (60, 40, 0, 10)
        assert ctx.canvas_layout(I420, 10, 4, 12) == (72, 48, 60, 6) and ctx.canvas_layout(YV12, 10, 6, 10) == (90, 60, 75, 5)
        assert ctx.canvas_layout(I420, 1920, 1080, 1920) == (1920 * 1080 * 3 // 2, 1920 * 1080, 1920 * 1080 * 5 // 4, 960)
        for args in ((1, 8, 8, 16), (2, 8, 8, 16), (3, 8, 8, 16), (8, 8, 8, 8), (-1, 8, 8, 8),                # packed 4:2:2 and unknown formats
                     (NV12, 7, 8, 8), (NV12, 8, 7, 8), (I420, 0, 8, 8), (YV12, 8, 0, 8), (NV12, 8, 8, 7),       # odd or empty sizes, a short stride
                     (I420, 8, 8, 9), (I420, 8, 8, 6), (BGR, 8, 8, 23), (BGR, 0, 8, 24)):
            assert emu.lvm_canvas_layout(*args, None, None, None, None) == INVALID, args
        assert emu.lvm_canvas_layout(NV12, 8, 8, 8, None, None, None, None) == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_shapes_emu(lvm, emu, fmt):
    _check_shapes(lvm, emu, HostMem(), fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_shapes_gpu(lvm, hip, fmt):
    _check_shapes(lvm, hip, TorchMem(), fmt)


# ---- 4. export ----------------------------------------------------------------------------------------------------------------------------
# (w, h, downscale, roi): pane sizes 10 x 6, 12 x 8 (ROI (2, 2) 24 x 16), 8 x 6, 6 x 6, 20 x 12 out of an ODD frame (21 x 13: crop-only, a row
# stride of 63 bytes) and 16 x 8 (left-right: pane 1 at x = 16, the one geometry whose fused conversion may take dword-wide loads)
EXPORT_GEOMETRY = [(20, 12, 2, None), (36, 22, 2, (2 / 36, 2 / 22, 24 / 36, 16 / 22)), (16, 12, 2, None), (12, 12, 2, None), (21, 13, 1, None), (16, 8, 1, None)]
SOURCES = [(3, False), (1, False), (3, True)]                     # colour; gray; the gray tap: a colour original beside a gray processed pane


def _none(lvm):
    return lvm.LvmParams(3, 1, 0, 0, 0, 0, 0, 30.0, 0)            # mode None: the chain hands the preprocessed frame on


def _labels(po, cw, chh):
    """one caption that starts at an odd pixel and ends inside 2 x 2 blocks on every side (clipped to the canvas like drawLabel's rectangle)"""
    return [po.standin_label_tables(9, 3, 1, 3, 1, cw, chh, seed=11)]


def _variants(ctx):
    return ctx.profile_variants().get("canvas_yuv", set())


def _check_export(lvm, po, lib, fmt, monkeypatch):
    """mode None: per geometry, source and split the canvases of each route against the restatement of the BGR context's canvases"""
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    pane_widths, vec_seen = set(), False
    try:
        a.set_canvas_format(fmt)
        a.profile(True)
        for gi, (w, h, ds, roi) in enumerate(EXPORT_GEOMETRY):
            for ch, gray in SOURCES:
                cpre, _ = _params(lvm, po, ds, roi, gray)
                frames = [_frame(w, h, ch, 3000 + 100 * gi + 10 * ch + t) for t in range(5)]      # sub-batches of 2, 2 and a remainder of 1
                for split in (NONE, LR, TB):
                    tag = (NAMES[fmt], (w, h, ds), (ch, gray), split)
                    a.export_set_overlay([]); b.export_set_overlay([])
                    ref, pb = b.export_frames(frames, cpre, _none(lvm), split)
                    chh, cw = ref[0].shape[:2]
                    pane_w = cw // 2 if split == LR else cw
                    if split == LR:
                        pane_widths.add(pane_w)
                    a.profile_only("canvas_yuv")
                    got, pa = a.export_frames(frames, cpre, _none(lvm), split)
                    assert pa == pb == [False] * 5, tag
                    for k in range(5):
                        assert got[k].shape == (chh * 3 // 2, cw) and np.array_equal(got[k], as_mat(ref[k], fmt)), tag + (k, "fused")
                    v = _variants(a)
                    assert "fused" in v and v - {"fused"} in ({"vec8"}, {"bytes"}), (tag, v)
                    if cw % 8 or (split == LR and pane_w % 8):
                        assert "vec8" not in v, (tag, v)          # pane 1 starts at x = pane_w: no multiple of 8, no dword-wide block loads
                    vec_seen = vec_seen or "vec8" in v
                    # the same frames through compose -> convert: equal bytes, and the fused route did not run
                    monkeypatch.setenv("LVM_CANVAS_FUSED", "0")
                    a.profile_only("canvas_yuv")
                    again, pa = a.export_frames(frames, cpre, _none(lvm), split)
                    monkeypatch.delenv("LVM_CANVAS_FUSED")
                    assert all(np.array_equal(x, y) for x, y in zip(again, got)) and pa == pb, tag
                    assert "fused" not in _variants(a) and _variants(a), (tag, _variants(a))
                    # with a label: compose, overlay, convert -- the label is applied to the BGR pixels first
                    labels = _labels(po, cw, chh)
                    a.export_set_overlay(labels); b.export_set_overlay(labels)
                    ref2, _ = b.export_frames(frames, cpre, _none(lvm), split)
                    assert not np.array_equal(ref2[0], ref[0])
                    a.profile_only("canvas_yuv")
                    got2, pa = a.export_frames(frames, cpre, _none(lvm), split)
                    assert pa == pb, tag
                    for k in range(5):
                        assert np.array_equal(got2[k], as_mat(ref2[k], fmt)), tag + (k, "label")
                    assert "fused" not in _variants(a) and _variants(a), (tag, _variants(a))
        assert {6, 8, 10, 12} <= pane_widths and vec_seen, (pane_widths, vec_seen)
    finally:
        a.close(); b.close()


def _check_export_clip(lvm, po, lib, fmt, source_fmt=BGR):
    """a short Laplace clip, split left-right, 7 frames (sub-batches of 2, 2, 2, 1): produced[] and bytes against the BGR context; with
    source_fmt the frames go IN as NV12 as well"""
    ck, pk = lvm.synth.config(0, (96, 64, 3))
    clip = lvm.synth.Clip(seed=42, **ck)
    frames = [clip.frame(t) for t in range(7)]
    raws = frames
    if source_fmt != BGR:
        raws = [raw_from_bgr(f, source_fmt) for f in frames]
        frames = [to_bgr(r, source_fmt) for r in raws]
    cpre, _ = _params(lvm, po, 1, (7 / 96, 5 / 64, 0.75, 0.75), False)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        a.set_canvas_format(fmt)
        a.set_source_format(source_fmt)
        got, pa = a.export_frames(raws, cpre, c_params(lvm, pk), LR)
        ref, pb = b.export_frames(frames, cpre, c_params(lvm, pk), LR)
        assert pa == pb and any(pa)
        for k in range(7):
            assert np.array_equal(got[k], as_mat(ref[k], fmt)), (NAMES[fmt], k)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_export_emu(lvm, po, emu, fmt, monkeypatch):
    _check_export(lvm, po, emu, fmt, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_export_gpu(lvm, po, hip, fmt, monkeypatch):
    _check_export(lvm, po, hip, fmt, monkeypatch)


def test_export_clip_emu(lvm, po, emu):
    _check_export_clip(lvm, po, emu, I420)
    _check_export_clip(lvm, po, emu, NV12, NV12)


@pytest.mark.gpu
def test_export_clip_gpu(lvm, po, hip):
    _check_export_clip(lvm, po, hip, I420)
    _check_export_clip(lvm, po, hip, NV12, NV12)


# ---- 5. default and back, refusals ---------------------------------------------------------------------------------------------------------
def _check_default_and_back(lvm, po, lib, mem):
    """under LVM_PIX_BGR the bytes, the launch names and the variants of lvm_export_frames and lvm_compose_device are the same before and after a
    round trip through NV12; lvm_reset keeps the format"""
    ck, pk = lvm.synth.config(0, (96, 64, 3))
    clip = lvm.synth.Clip(seed=5, **ck)
    frames = [clip.frame(t) for t in range(5)]
    cpre, _ = _params(lvm, po, 2, None, False)
    orig, proc = _frame(24, 16, 3, 1), _frame(24, 16, 1, 2)
    ctx = lvm.Context(0, 1, lib)

    def run():
        ctx.reset()
        ctx.profile_only(None)
        canv, produced = ctx.export_frames(frames, cpre, c_params(lvm, pk), LR)
        d_o, d_p, d_c = mem.upload(orig), mem.upload(proc), mem.upload(np.zeros((16, 48, 3), np.uint8))
        ctx.compose_device(LR, ctypes.c_void_p(mem.ptr_at(d_o.reshape(-1), 0)), 24, 16, 3, 72, 72 * 16, ctypes.c_void_p(mem.ptr_at(d_p.reshape(-1), 0)), 24, 16, 1, 24, 24 * 16,
                           ctypes.c_void_p(mem.ptr_at(d_c.reshape(-1), 0)), 144, 144 * 16, mem.stream())
        mem.sync(ctx)
        return canv, produced, mem.download(d_c).copy(), sorted(ctx.profile_collect()), ctx.profile_variants()

    try:
        ctx.profile(True)
        assert ctx.canvas_format() == BGR
        before = run()
        assert "canvas_yuv" not in before[3] and "compose" in before[3]
        ctx.set_canvas_format(NV12)
        ctx.reset()
        assert ctx.canvas_format() == NV12                          # lvm_reset keeps the format
        nv, _ = ctx.export_frames(frames, cpre, c_params(lvm, pk), LR)
        assert nv[0].shape == (before[0][0].shape[0] * 3 // 2, before[0][0].shape[1])
        ctx.set_canvas_format(BGR)
        after = run()
        assert before[1] == after[1] and all(np.array_equal(x, y) for x, y in zip(before[0], after[0]))
        assert np.array_equal(before[2], after[2]) and before[3] == after[3] and before[4] == after[4]
    finally:
        ctx.close()


def _check_refusals(lvm, po, lib, mem):
    """every refusal is LVM_ERR_INVALID with a message that names the rule, writes nothing and changes no state: the NV12 clip of a context that
    is refused every way in its middle goes on like its undisturbed twin's"""
    ck, pk = lvm.synth.config(0, (96, 64, 3))
    clip = lvm.synth.Clip(seed=9, **ck)
    cpre, cp = lvm.to_c_preprocess(lvm.PreprocessParams(), False), c_params(lvm, pk)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    msg = lambda: lib.lvm_last_error(a.h).decode()
    w, h = 16, 8
    d_in = mem.upload(np.full(2 * w * h * 3 + 64, 0x11, np.uint8))
    d_out = mem.upload(np.full(4 * w * h + 64, 0xCD, np.uint8))
    pi, po_ = ctypes.c_void_p(mem.ptr_at(d_in, 0)), ctypes.c_void_p(mem.ptr_at(d_out, 0))

    def convert_refused(match, fmt=NV12, w=w, h=h, bstride=w * 3, n=1, stride=w, ofs=w * h * 3 // 2):
        rc = lib.lvm_canvas_convert_device(a.h, fmt, pi, w, h, bstride, bstride * max(h, 1), n, po_, stride, ofs, mem.stream())
        assert rc == INVALID and match in msg(), (rc, match, msg())

    def export_refused(match, frame, stride):
        canvas = np.full(64 * 96 * 3, 0xCD, np.uint8)
        pin, pout, produced = (ctypes.c_void_p * 1)(frame.ctypes.data), (ctypes.c_void_p * 1)(canvas.ctypes.data), (ctypes.c_int * 1)(7)
        rc = lib.lvm_export_frames(a.h, ctypes.byref(cpre), ctypes.byref(cp), NONE, 1, pin, 96, 64, 3, 96 * 3, pout, stride, produced)
        assert rc == INVALID and match in msg() and (canvas == 0xCD).all(), (rc, match, msg())

    try:
        for ctx in (a, b):
            ctx.set_canvas_format(NV12)
        for t in range(8):
            f = clip.frame(t)
            if t == 4:
                for bad in (1, 2, 3, 8, -1):                       # the packed 4:2:2 formats are no canvas formats
                    assert lib.lvm_set_canvas_format(a.h, bad) == INVALID
                    assert "lvm_set_canvas_format" in msg() and "(0)" in msg() and "(4)" in msg() and "(7)" in msg()
                    assert a.canvas_format() == NV12                # an unknown format changes nothing
                convert_refused("LVM_PIX_NV12 (4)", fmt=BGR)
                convert_refused("LVM_PIX_NV12 (4)", fmt=2)
                convert_refused("must be even", w=15)
                convert_refused("must be even", h=7)
                convert_refused("must be even", h=0)
                convert_refused("bgr_stride must be >= 3 * w", bstride=w * 3 - 1)
                convert_refused("canvas_stride must be >= canvas_w", stride=w - 1)
                convert_refused("canvas_stride must be even", fmt=I420, stride=w + 1)
                convert_refused("canvas_stride must be even", fmt=YV12, stride=w - 2)
                convert_refused("overlap", n=2, ofs=w * h * 3 // 2 - 1)
                mem.sync(a)
                assert (mem.download(d_out) == 0xCD).all()
                export_refused("canvas_stride must be >= canvas_w", f, 95)
                a.set_canvas_format(I420)
                export_refused("canvas_stride must be even", f, 97)
                a.set_canvas_format(NV12)
            ca, pa = a.export_frames([f], cpre, cp, NONE)
            cb, pb = b.export_frames([f], cpre, cp, NONE)
            assert pa == pb, t
            assert np.array_equal(ca[0], cb[0]), t                  # (a temporal state reset by a refusal would show here)
    finally:
        a.close(); b.close()


def test_default_and_back_emu(lvm, po, emu):
    _check_default_and_back(lvm, po, emu, HostMem())


def test_refusals_emu(lvm, po, emu):
    _check_refusals(lvm, po, emu, HostMem())


@pytest.mark.gpu
def test_default_and_refusals_gpu(lvm, po, hip):
    _check_default_and_back(lvm, po, hip, TorchMem())
    _check_refusals(lvm, po, hip, TorchMem())


# ---- 6. call order across streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_convert_sees_the_compose_of_another_stream_gpu(lvm, hip):
    """lvm_canvas_convert_device on a stream other than the preceding lvm_compose_device's: calls of one context take effect in call order"""
    import torch
    w, h = 1920, 1080
    orig, proc = _frame(w, h, 3, 61), _frame(w, h, 1, 62)
    canvas = np.concatenate([orig, np.repeat(proc[:, :, None], 3, axis=2)], axis=1)
    want = bgr2yuv420(canvas, NV12)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    d_o, d_p = torch.from_numpy(orig).cuda(), torch.from_numpy(proc).cuda()
    d_c = torch.zeros((h, 2 * w, 3), dtype=torch.uint8, device="cuda")
    d_y = torch.full((want.size,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx = lvm.Context(0, 1, hip)
    try:
        ctx.compose_device(LR, ctypes.c_void_p(d_o.data_ptr()), w, h, 3, w * 3, w * h * 3, ctypes.c_void_p(d_p.data_ptr()), w, h, 1, w, w * h, ctypes.c_void_p(d_c.data_ptr()),
                           2 * w * 3, 2 * w * h * 3, s1.cuda_stream)
        ctx.canvas_convert_device(NV12, ctypes.c_void_p(d_c.data_ptr()), 2 * w, h, 2 * w * 3, 2 * w * h * 3, 1, ctypes.c_void_p(d_y.data_ptr()), 2 * w, want.size, s2.cuda_stream)
        s2.synchronize()
        assert np.array_equal(d_y.cpu().numpy(), want)
    finally:
        ctx.close()


# ---- 7. the OpenCV boundary -----------------------------------------------------------------------------------------------------------------
def golden_bgr():
    """the fixed BGR frame of tools/pin_with_opencv.sh: 32 x 16, seed 9420"""
    return _frame(32, 16, 3, 9420)


@pytest.mark.refpin
def test_restatement_against_opencv_golden():
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/bgr2yuv_420.npz is absent: run tools/pin_with_opencv.sh where OpenCV 4 is installed")
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["bgr"], golden_bgr())
    assert np.array_equal(gold["i420"], as_mat(golden_bgr(), I420))
    assert np.array_equal(gold["yv12"], as_mat(golden_bgr(), YV12))
