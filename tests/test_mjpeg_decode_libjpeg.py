"""Motion-JPEG decode, libjpeg-exact kind (lvm_mjpeg_set_decoder(ctx, LVM_MJPEG_DECODER_LIBJPEG); csrc/mjpeg_decode.hip: k_mjd_chroma_islow,
k_mjd_pixels_libjpeg): the frames a libjpeg-backed `cv::VideoCapture::read` (source/FileSource.cpp:99) hands to the chain.

libjpeg's decode is deterministic integer work (islow IDCT, h2v2 fancy upsampling, the YCC tables), so the bar is EQUALITY everywhere in this file:
  tests/libjpeg_ref.py (numpy)  ==  Pillow (libjpeg-turbo, the independent decoder in the image)      -- pins the yardstick
  the HIP kernels               ==  both                                                              -- emulation build here, the GPU through the C ABI
and consequently a file -> file export and a Riesz magnification fed by the device decoder equal, byte for byte, the ones fed by Pillow's frames."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import libjpeg_ref as lj
from oracle import mjpeg_oracle as mo
from test_mjpeg import decode as pil_decode, texture
from test_mjpeg_decode import STREAMS, _numpy_alloc, _strip_dht, pil_encode

LIBJPEG, REPLICATE = 1, 0

# the grid the arithmetic of libjpeg_ref was established on: 1 x 1 up to an MCU row of 1080p, chroma planes of 1, 2 (libjpeg replicates) and 3 samples
# (the narrowest it filters), odd x odd sizes, the coarsest and the finest quantisers
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (4, 7), (3, 40), (5, 3), (6, 2), (5, 1), (8, 1), (1, 9), (2, 31), (7, 40), (16, 16), (17, 9), (18, 18), (31, 33),
         (33, 21), (47, 15), (64, 48), (100, 70), (130, 34), (1920, 24)]
QUALITIES = (1, 10, 30, 50, 75, 90, 95, 100)


def _sources(w, h, q, rng):
    return [texture(w, h, seed=w + h + q), rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            np.where(rng.random((h, w, 1)) < .5, 0, 255).astype(np.uint8).repeat(3, 2)]


def _four_streams(f, q):
    return [pil_encode(f, q, subsampling=2), pil_encode(f, q, subsampling=2, optimize=True), mo.encode_frame(f, q), mo.encode_frame(f, q, restart=3)]


@pytest.mark.parametrize("w,h", SIZES)
def test_libjpeg_ref_is_what_pillow_decodes(w, h):
    """the yardstick: numpy restatement == Pillow's libjpeg-turbo, byte for byte, on every size x quality x source (texture, uniform noise, 0 / 255
    noise) x stream (Pillow's, Pillow's with optimised Huffman tables, this encoder's, this encoder's with restart intervals of 3 MCUs)"""
    rng = np.random.default_rng(1000 * w + h)
    for q in QUALITIES:
        for si, f in enumerate(_sources(w, h, q, rng)):
            for k, j in enumerate(_four_streams(f, q)):
                mine, theirs = lj.decode(j), pil_decode(j)
                assert mine.shape == theirs.shape == f.shape
                d = np.abs(mine.astype(int) - theirs)
                assert not d.any(), "%dx%d q%d source %d stream %d: %d bytes differ, by up to %d" % (w, h, q, si, k, int((d > 0).sum()), int(d.max()))


def test_libjpeg_ref_stages():
    """the stages libjpeg_ref exposes fit together, and the narrow-plane rule is the one libjpeg applies: at w = 4 (chroma 2 wide) the filter is off,
    at w = 5 (3 wide) it is on -- the filtered variant of the narrow plane would NOT be Pillow's frame"""
    f = texture(4, 16, seed=3)
    f[:, :2], f[:, 2:] = (250, 20, 30), (10, 240, 200)                                 # two chroma columns far apart
    j = pil_encode(f, 95, subsampling=2)
    hd, planes = lj.idct_planes(j)
    cb, cr = lj.chroma_planes(hd, planes)
    assert cb.shape == cr.shape == (8, 2) and lj.luma_plane(planes).shape == (16, 16)
    assert np.array_equal(lj.upsample(cb), np.repeat(np.repeat(cb, 2, 0), 2, 1))
    assert np.array_equal(lj.bgr(hd, lj.luma_plane(planes), lj.upsample(cb), lj.upsample(cr)), pil_decode(j))
    assert not np.array_equal(lj.bgr(hd, lj.luma_plane(planes), mo.upsample_fancy(cb), mo.upsample_fancy(cr)), pil_decode(j))
    hd5, planes5 = lj.idct_planes(pil_encode(texture(5, 16, seed=3), 95, subsampling=2))
    cb5 = lj.chroma_planes(hd5, planes5)[0]
    assert cb5.shape == (8, 3) and np.array_equal(lj.upsample(cb5), mo.upsample_fancy(cb5))


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------------------
SMALL = STREAMS + [(3, 5, 75), (4, 7, 90), (31, 33, 60)]


def _batch(w, h, q):
    """every kind of stream, two sets of quantiser tables in one batch"""
    f = texture(w, h, seed=w + h)
    f2 = texture(w, h, seed=w + h + 5)
    q2 = max(1, q - 20)
    return [mo.encode_frame(f, q), mo.encode_frame(f, q, restart=3), _strip_dht(mo.encode_frame(f, q)), pil_encode(f, q, subsampling=2),
            pil_encode(f, q, subsampling=2, optimize=True), mo.encode_frame(f2, q2), pil_encode(f2, q2, subsampling=2)]


def _decode_and_compare(lvm, lib, alloc, read, cases, ref=True):
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
        for (w, h, q) in cases:
            js = _batch(w, h, q)
            row = w * 3 + (5 if w % 2 else 8)                                          # padded rows, odd and even pitches
            buf = alloc(len(js), h, row)
            ctx.mjpeg_decode_device(js, w, h, buf[0], stride=row, frame_stride=row * h)
            got = read(buf)
            for k, j in enumerate(js):
                mine = got[k, :, :w * 3].reshape(h, w, 3)
                theirs = pil_decode(j)
                d = np.abs(mine.astype(int) - theirs)
                assert not d.any(), "%dx%d q%d stream %d against Pillow: %d bytes differ, by up to %d" % (w, h, q, k, int((d > 0).sum()), int(d.max()))
                if ref:
                    assert np.array_equal(mine, lj.decode(j)), "%dx%d q%d stream %d against libjpeg_ref" % (w, h, q, k)
                assert (got[k, :, w * 3:] == 0xEE).all(), "%dx%d q%d stream %d: padding bytes written" % (w, h, q, k)
    finally:
        ctx.close()


def test_libjpeg_kind_emu_byte_identical_to_pillow(lvm, emu):
    _decode_and_compare(lvm, emu, *_numpy_alloc(), SMALL)


def test_libjpeg_kind_emu_narrow_and_ragged_sizes(lvm, emu):
    """chroma planes of 1, 2, 3 samples in either direction, frames of one pixel row / column, more than sixteen MCUs per row (two workgroups of
    k_mjd_chroma_islow) and a last wave with fewer than four MCUs"""
    _decode_and_compare(lvm, emu, *_numpy_alloc(), [(2, 2, 75), (4, 4, 50), (5, 3, 95), (6, 2, 75), (5, 1, 90), (8, 1, 75), (1, 9, 75), (2, 31, 30),
                                                    (3, 40, 85), (7, 40, 100), (47, 15, 1), (18, 18, 10), (290, 20, 80), (337, 17, 92)])


def test_libjpeg_kind_emu_both_entropy_paths():
    """as tests/test_mjpeg_decode.py: this file again with every frame without restart markers sent through the self-synchronising kernels
    (LVM_MJD_PARALLEL=2) and none (=0) -- the arithmetic behind them sees the same coefficients (the switch is read once per process)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode in ("2", "0"):
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "tests/test_mjpeg_decode_libjpeg.py", "-m", "not gpu", "-k", "emu and not both_entropy_paths"],
                           capture_output=True, text=True, env=dict(os.environ, LVM_MJD_PARALLEL=mode), cwd=root, timeout=900)
        assert r.returncode == 0 and "passed" in r.stdout, (mode, (r.stdout + r.stderr)[-3000:])


def test_libjpeg_kind_emu_the_switch_changes_the_arithmetic_only(lvm, emu):
    ctx = lvm.Context(0, 1, emu)
    try:
        w, h = 66, 38
        f = texture(w, h, seed=9)
        js = [mo.encode_frame(f, 85), pil_encode(f, 85, subsampling=2)]
        out = np.zeros((2, h, w, 3), np.uint8)
        p = ctypes.c_void_p(out.ctypes.data)

        def run():
            out[...] = 0
            ctx.mjpeg_decode_device(js, w, h, p)
            return out.copy()
        was = run()
        assert all(np.array_equal(was[k], mo.decode_frame(j)) for k, j in enumerate(js))           # the default is the replicating decoder
        ctx.mjpeg_set_decoder(LIBJPEG)
        got = run()
        assert all(np.array_equal(got[k], pil_decode(j)) for k, j in enumerate(js)) and not np.array_equal(got, was)
        for bad in (2, -1, 7):
            with pytest.raises(lvm.LvmError, match="lvm_mjpeg_set_decoder"):
                ctx.mjpeg_set_decoder(bad)
        assert np.array_equal(run(), got)                                                          # a refused kind changes nothing
        ctx.mjpeg_set_decoder(REPLICATE)
        assert np.array_equal(run(), was)
        # what the kind does not touch: the refusals of the parser
        ctx.mjpeg_set_decoder(LIBJPEG)
        with pytest.raises(lvm.LvmError, match="4:2:0"):
            ctx.mjpeg_decode_device([pil_encode(f, 80, subsampling=0)], w, h, p)
        with pytest.raises(lvm.LvmError, match="size"):
            ctx.mjpeg_decode_device([mo.encode_frame(texture(32, 48), 80)], w, h, p)
        assert np.array_equal(run(), got)
    finally:
        ctx.close()


def test_libjpeg_kind_emu_survives_corrupted_streams(lvm, emu):
    """the damage of tests/test_mjpeg_decode.py::test_mjpeg_decode_emu_survives_corrupted_streams under the libjpeg kind: coefficients no encoder
    produces go through the unclamped dequantiser and the wrap-around IDCT -- the call decodes something or fails with a message, and the context
    decodes the intact streams exactly afterwards (tools/emu_asan.sh and tools/emu_ubsan.sh run this file under the sanitizers)"""
    rng = np.random.default_rng(3)
    f = texture(96, 64)
    streams = [mo.encode_frame(f, 85), mo.encode_frame(f, 85, restart=2), pil_encode(f, 85, subsampling=2)]
    ctx = lvm.Context(0, 1, emu)
    try:
        ctx.mjpeg_set_decoder(LIBJPEG)
        out = np.zeros((1, 64, 96 * 3), np.uint8)
        p = ctypes.c_void_p(out.ctypes.data)
        failed = 0
        for t in range(90):
            j = bytearray(streams[t % 3])
            kind = t % 5
            if kind == 0:                                            # a few flipped bytes in the entropy-coded segment
                for _ in range(1 + t % 4):
                    j[int(rng.integers(len(j) // 2, len(j) - 2))] = int(rng.integers(0, 256))
            elif kind == 1:                                          # ... anywhere behind SOI
                j[int(rng.integers(2, len(j)))] ^= 1 << int(rng.integers(0, 8))
            elif kind == 2:                                          # truncated
                del j[int(rng.integers(20, len(j))):]
            elif kind == 3:                                          # a restart marker where none belongs
                k = int(rng.integers(len(j) // 2, len(j) - 4))
                j[k:k + 2] = b"\xff" + bytes([0xD0 + t % 8])
            else:                                                    # entropy data replaced by noise
                hd = mo.parse_header(bytes(j))
                j[hd["data_start"]:-2] = rng.integers(0, 256, len(j) - 2 - hd["data_start"], dtype=np.uint8).tobytes()
            try:
                ctx.mjpeg_decode_device([bytes(j)], 96, 64, p)
            except lvm.LvmError as e:
                failed += 1
                assert "lvm_mjpeg_decode" in str(e)
        assert failed > 10
        # the largest coefficients the entropy layer can carry (16-bit tables are refused, so |coef * q| < 2^23): defined, whatever they decode to
        big = bytearray(mo.encode_frame(f, 100))
        i = big.index(b"\xff\xdb")
        big[i + 5:i + 5 + 64] = bytes([255] * 64)
        ctx.mjpeg_decode_device([bytes(big)], 96, 64, p)
        for j in streams:
            ctx.mjpeg_decode_device([j], 96, 64, p)
            assert np.array_equal(out[0].reshape(64, 96, 3), pil_decode(j))
    finally:
        ctx.close()


def _transcode_case(lvm, lib, w, h, n, split, pre_kw, q_in, q_out):
    """lvm_export_mjpeg_frames under the libjpeg kind == decode (Pillow) -> lvm_export_frames -> encode (oracle), byte for byte"""
    from helpers import c_params
    ck, pk = lvm.synth.config(0)
    clip = lvm.synth.Clip(seed=7, **dict(ck, w=w, h=h))
    jin = [mo.encode_frame(clip.frame(t), q_in) if t % 2 else pil_encode(clip.frame(t), q_in, subsampling=2) for t in range(n)]     # both kinds of stream
    decoded = [pil_decode(j) for j in jin]
    pre = lvm.LvmPreprocessParams(1, 0, 0.0, 0.0, 1.0, 1.0, 0)
    for k, v in pre_kw.items():
        setattr(pre, k, v)
    cp = c_params(lvm, pk)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        b.mjpeg_set_decoder(LIBJPEG)
        canvases, prod_a = a.export_frames(decoded, pre, cp, split)
        jout, prod_b = b.export_mjpeg_frames(jin, w, h, pre, cp, split, quality=q_out)
        assert prod_a == prod_b
        for k in range(n):
            assert jout[k] == mo.encode_frame(canvases[k], q_out), "frame %d" % k
    finally:
        a.close()
        b.close()


ROI_MODES = {0: (6, {}), 2: (6, {}), 3: (22, {"framerate": 7.0, "coLow": 0.4, "coHigh": 2.0})}      # synth.config index -> frames, parameter overrides


def _roi_view_case(lvm, lib, idx):
    """The production path that hands the magnifier an unaligned view in temporal batches: a 75 x 53 source coded by libjpeg (Pillow, quality
    90, 4:2:0), decoded on the device, ROI only (downscale 1, no gray) -- the magnifier and compose_device's `orig` read
    d_decoded + ry * 225 + rx * 3 with rows of 225 bytes.  ROIs of 61 x 45 (odd size) and 64 x 48 (w % 4 == 0: only layout and pointer keep
    the vector kernels away) at (5, 3); split left | right.  Both contexts run OpenCV-order Lab: the second one magnifies the cropped frame
    from a packed upload, where it may take the vector kernels, and the bytes must not depend on that."""
    from helpers import c_params
    w, h = 75, 53
    n, over = ROI_MODES[idx]
    ck, pk = lvm.synth.config(idx, (w, h, 2))
    pk.update(over)
    clip = lvm.synth.Clip(seed=7, **ck)
    jin = [pil_encode(clip.frame(t), 90, subsampling=2) for t in range(n)]
    decoded = [pil_decode(j) for j in jin]
    cp = c_params(lvm, pk)
    for rw, rh in ((61, 45), (64, 48)):
        pre = lvm.LvmPreprocessParams(1, 1, 5.2 / 75, 3.2 / 53, rw / 75, rh / 53, 0)
        a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
        try:
            # (a change in the geometry's rounding must not silently re-align the view)
            assert a.preprocess_geometry(pre, w, h, 3) == (5, 3, rw, rh, rw, rh, 3)
            a.exact_lab(True)
            b.exact_lab(True)
            b.mjpeg_set_decoder(LIBJPEG)
            canvases, prod_a = a.export_frames(decoded, pre, cp, 1)
            jout, prod_b = b.export_mjpeg_frames(jin, w, h, pre, cp, 1, quality=85)
            assert prod_a == prod_b and any(prod_a)
            for k in range(n):
                assert jout[k] == mo.encode_frame(canvases[k], 85), "ROI %d x %d, frame %d" % (rw, rh, k)
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize("idx", [0, 2, 3])
def test_libjpeg_kind_emu_export_roi_view_in_batches(lvm, emu, idx):
    _roi_view_case(lvm, emu, idx)


def test_libjpeg_kind_emu_export_mjpeg_to_mjpeg(lvm, emu):
    _transcode_case(lvm, emu, 66, 38, 6, 1, {}, 90, 80)
    _transcode_case(lvm, emu, 80, 60, 5, 2, dict(downscale=2, roi_enabled=1, roiX=0.1, roiY=0.2, roiW=0.7, roiH=0.6, grayscale=1), 85, 95)
    _transcode_case(lvm, emu, 64, 48, 3, 0, dict(roi_enabled=1, roiX=0.25, roiY=0.25, roiW=0.5, roiH=0.5), 85, 75)     # ROI only: the magnifier reads a view of the decoded frame
    _transcode_case(lvm, emu, 160, 96, 4, 1, {}, 97, 85)                # libjpeg's frames of > 2 KB: the self-synchronising kernels in front


# ---- the GPU -------------------------------------------------------------------------------------------------------------------------------------
def _torch_alloc():
    import torch

    def alloc(n, h, row):
        t = torch.full((n, h, row), 0xEE, dtype=torch.uint8, device="cuda")
        return (ctypes.c_void_p(t.data_ptr()), t)
    return alloc, (lambda b: b[1].cpu().numpy())


@pytest.mark.gpu
def test_libjpeg_kind_gpu_byte_identical_to_pillow(lvm, hip):
    _decode_and_compare(lvm, hip, *_torch_alloc(), SMALL)
    _decode_and_compare(lvm, hip, *_torch_alloc(), [(640, 360, 90), (322, 182, 75)], ref=False)       # (the numpy entropy decoder takes minutes at these sizes)


@pytest.mark.gpu
def test_libjpeg_kind_gpu_1080p(lvm, hip):
    """four 1080p frames at quality 90 as this encoder writes them (restart intervals of 8 MCUs: a lane per interval) and as libjpeg does (no
    markers: the self-synchronising kernels): every byte of every frame is Pillow's"""
    import torch
    w, h, n = 1920, 1080, 4
    f = np.stack([texture(w, h, seed=k) for k in range(n)])
    ctx = lvm.Context(0, 1, hip)
    try:
        d = torch.from_numpy(f).cuda()
        mine = ctx.mjpeg_encode_device(ctypes.c_void_p(d.data_ptr()), w, h, n, quality=90)
        assert mo.parse_header(mine[0])["restart"] == 8
        theirs = [pil_encode(f[k], 90, subsampling=2) for k in range(n)]
        assert mo.parse_header(theirs[0])["restart"] == 0
        ctx.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
        out = torch.zeros_like(d)
        for name, js in (("this encoder's", mine), ("libjpeg's", theirs)):
            out.zero_()
            ctx.mjpeg_decode_device(js, w, h, ctypes.c_void_p(out.data_ptr()))
            got = out.cpu().numpy()
            for k in range(n):
                dd = np.abs(got[k].astype(int) - pil_decode(js[k]))
                assert not dd.any(), "%s frame %d: %d bytes differ, by up to %d" % (name, k, int((dd > 0).sum()), int(dd.max()))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_libjpeg_kind_gpu_export_mjpeg_to_mjpeg(lvm, hip):
    _transcode_case(lvm, hip, 640, 360, 9, 1, {}, 90, 85)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 2, 3])
def test_libjpeg_kind_gpu_export_roi_view_in_batches(lvm, hip, idx):
    _roi_view_case(lvm, hip, idx)


@pytest.mark.gpu
def test_libjpeg_kind_gpu_riesz_end_to_end(lvm, hip):
    """BASELINE config 2 (Riesz, alpha 50 on the phase) at 320 x 180 for 16 frames of a libjpeg-coded source: decoded on the device under the libjpeg
    kind and magnified there == decoded by Pillow, uploaded and magnified on a second context, byte for byte.  Under the replicating kind the two
    magnified sequences are 39.7 dB apart with single pixels 89 levels off (tests/test_mjpeg_decode.py::test_chroma_upsampling_variant_through_the_
    magnifier); for a libjpeg-backed capture that divergence is gone."""
    import torch
    from helpers import c_params
    w, h, n = 320, 180, 16
    ck, pk = lvm.synth.config(2, (w, h, 5))
    clip = lvm.synth.Clip(**ck)
    cp = c_params(lvm, pk)
    js = [pil_encode(clip.frame(t), 90, subsampling=2) for t in range(n)]
    fb = w * h * 3
    st = torch.cuda.current_stream().cuda_stream
    a, b = lvm.Context(0, 1, hip), lvm.Context(0, 1, hip)
    try:
        a.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
        d_in = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
        a.mjpeg_decode_device(js, w, h, ctypes.c_void_p(d_in.data_ptr()))
        d_out = torch.zeros_like(d_in)
        prod_a = a.process_device_frames(cp, n, d_in.data_ptr(), w, h, 3, w * 3, fb, fb, d_out.data_ptr(), w * 3, fb, fb, st)
        torch.cuda.synchronize()
        u_in = torch.from_numpy(np.stack([pil_decode(j) for j in js])).cuda()
        assert torch.equal(d_in, u_in), "the decoded inputs differ"
        u_out = torch.zeros_like(u_in)
        prod_b = b.process_device_frames(cp, n, u_in.data_ptr(), w, h, 3, w * 3, fb, fb, u_out.data_ptr(), w * 3, fb, fb, st)
        torch.cuda.synchronize()
        assert list(prod_a) == list(prod_b) and any(prod_a)
        ga, gb = d_out.cpu().numpy(), u_out.cpu().numpy()
        for t in range(n):
            if prod_a[t]:
                dd = np.abs(ga[t].astype(int) - gb[t])
                assert not dd.any(), "magnified frame %d: %d bytes differ, by up to %d" % (t, int((dd > 0).sum()), int(dd.max()))
    finally:
        a.close()
        b.close()


# ---- the host shims pass the kind through -----------------------------------------------------------------------------------------------------------
SHIM_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lvm_hip.h"
#include "HipExportRunner.hpp"
#include "HipMjpegWriter.hpp"
struct Traits {      // (the runner's loop is not run here: its context decodes)
    struct View { const std::uint8_t* data; int w, h, channels; std::ptrdiff_t stride; bool empty; };
    struct Source {}; struct Sink {};
    static bool next(Source&, View&) { return false; }
    static bool write(Sink&, std::uint64_t, std::int64_t, std::uint8_t*, int, int, std::ptrdiff_t) { return true; }
    static bool write_jpeg(Sink&, std::uint64_t, std::int64_t, const std::uint8_t*, std::size_t, int, int) { return true; }
    static bool aborted(const Sink&) { return false; }
};
int main(int argc, char** argv) {       // blob of JPEG frames, AVI path, output path, w, h, then the frame sizes
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]), n = argc - 6;
    std::FILE* f = std::fopen(argv[1], "rb");
    lvm::MjpegAviWriter wr;
    if (!f || !wr.open(argv[2], w, h, 25.0)) return 2;
    for (int k = 0; k < n; ++k) {
        std::vector<std::uint8_t> j((size_t)std::atoi(argv[6 + k]));
        if (std::fread(j.data(), 1, j.size(), f) != j.size() || !wr.write(j.data(), j.size())) return 3;
    }
    std::fclose(f);
    if (!wr.close()) return 4;
    lvm::MjpegAviReader plain, rd(LVM_MJPEG_DECODER_LIBJPEG);
    if (plain.decoder() != LVM_MJPEG_DECODER_REPLICATE || rd.decoder() != LVM_MJPEG_DECODER_LIBJPEG || !rd.open(argv[2]) || rd.frames() != (size_t)n) return 5;
    lvm::ExportRunner<Traits> runner(0, 4);
    bool refused = false;
    try { runner.set_mjpeg_decoder(5); } catch (const lvm::Error& e) { refused = e.status() == LVM_ERR_INVALID; }
    if (!refused) return 6;
    runner.set_mjpeg_decoder(rd.decoder());
    std::vector<std::uint8_t> bytes;
    std::vector<size_t> offs(1, 0);
    for (int k = 0; k < n; ++k) {
        bytes.resize(offs.back() + rd.frame_bytes((size_t)k));
        if (!rd.read((size_t)k, bytes.data() + offs.back())) return 7;
        offs.push_back(bytes.size());
    }
    void* out = nullptr;                    // (page-locked host memory: device-accessible on the GPU, plain memory in the emulation build)
    if (lvm_host_alloc((size_t)n * w * h * 3, &out) != LVM_OK) return 8;
    if (lvm_mjpeg_decode_device(runner.handle(), bytes.data(), offs.data(), n, w, h, (std::uint8_t*)out, (std::ptrdiff_t)w * 3, (std::ptrdiff_t)w * 3 * h) != LVM_OK) {
        std::printf("%s\n", lvm_last_error(runner.handle()));
        return 9;
    }
    std::FILE* o = std::fopen(argv[3], "wb");
    const bool ok = o && std::fwrite(out, 1, (size_t)n * w * h * 3, o) == (size_t)n * w * h * 3 && std::fclose(o) == 0;
    lvm_host_free(out);
    return ok ? 0 : 10;
}
"""


def test_libjpeg_kind_emu_through_the_host_shims(tmp_path, emu):
    """host/HipMjpegWriter.hpp's reader carries the kind, host/HipExportRunner.hpp applies it to its context (lvm::Magnifier::mjpeg_set_decoder):
    frames written into an AVI file, found again and decoded on the runner's context are Pillow's; an unknown kind throws lvm::Error"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h, n = 50, 34, 3
    js = [pil_encode(texture(w, h, seed=k), 88, subsampling=2) for k in range(n)]
    (tmp_path / "frames.bin").write_bytes(b"".join(js))
    (tmp_path / "t.cpp").write_text(SHIM_SRC)
    libdir = os.path.join(root, "tests", "emu", "_build")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", str(tmp_path / "t.cpp"), "-I", os.path.join(root, "include"),
                           "-I", os.path.join(root, "live-video-magnification_amd", "host"), "-L", libdir, "-llvm_emu", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "t")])
    r = subprocess.run([str(tmp_path / "t"), str(tmp_path / "frames.bin"), str(tmp_path / "a.avi"), str(tmp_path / "out.bin"), str(w), str(h)] + [str(len(j)) for j in js],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(n, h, w, 3)
    for k in range(n):
        assert np.array_equal(got[k], pil_decode(js[k])), "frame %d" % k
