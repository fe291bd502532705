"""Motion-JPEG decode of the samplings a baseline file can have besides 4:2:0 (lvm_mjpeg_set_samplings; csrc/mjpeg_decode.hip: the entropy layer with
the MCU as a property of the call, k_mjd_pixels_direct for 4:4:4 and gray, k_mjd_chroma_islow + k_mjd_pixels_h2v1 for 4:2:2): what UVC cameras,
FFmpeg's yuvj422p / yuvj444p and grayscale cameras write, decoded with libjpeg's arithmetic.

As in tests/test_mjpeg_decode_libjpeg.py the bar is EQUALITY everywhere:
  tests/libjpeg_ref_samplings.py (numpy)  ==  Pillow (libjpeg-turbo)      -- pins the yardstick
  the HIP kernels                         ==  both                        -- emulation build here, the GPU through the C ABI
and a file -> file export and a Riesz magnification fed by the device decoder equal, byte for byte, the ones fed by Pillow's frames."""
import ctypes
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import libjpeg_ref_samplings as ljs
from oracle import mjpeg_oracle as mo
from test_mjpeg import texture
from test_mjpeg_decode import _numpy_alloc, _strip_dht

PIL_Image = pytest.importorskip("PIL.Image")

LIBJPEG, REPLICATE = 1, 0
S420, S422, S444, GRAY, ALL = 1, 2, 4, 8, 15
NEW = (("4:2:2", S422), ("4:4:4", S444), ("gray", GRAY))
SUBSAMPLING = {S420: 2, S422: 1, S444: 0}


def enc(f, q, samp, **kw):
    """Pillow's (libjpeg-turbo's) stream of the BGR frame f in the given sampling; gray: its green plane as a one-component frame"""
    buf = io.BytesIO()
    if samp == GRAY:
        PIL_Image.fromarray(np.ascontiguousarray(f[..., 1])).save(buf, "JPEG", quality=q, **kw)
    else:
        PIL_Image.fromarray(f[..., ::-1]).save(buf, "JPEG", quality=q, subsampling=SUBSAMPLING[samp], **kw)
    return buf.getvalue()


def pil_decode(j):
    """what a libjpeg-backed cv::VideoCapture hands out: Pillow's frame as BGR (.convert("RGB") makes b = g = r of a one-component frame)"""
    im = PIL_Image.open(io.BytesIO(j))
    im.load()
    assert im.mode in ("RGB", "L")
    return np.asarray(im.convert("RGB"))[..., ::-1]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 2), (3, 5), (4, 4), (4, 7), (5, 3), (6, 2), (5, 1), (8, 1), (1, 9), (2, 31), (7, 40), (16, 16), (17, 9), (18, 18), (31, 33), (33, 21),
         (47, 15), (64, 48), (130, 34)]
QUALITIES = (1, 30, 75, 95, 100)
VARIANTS = ((S420, {}), (S422, {}), (S444, {}), (GRAY, {}), (S422, dict(restart_marker_blocks=3)), (S444, dict(restart_marker_blocks=2, optimize=True)),
            (GRAY, dict(restart_marker_blocks=5)))


def _assert_ref_is_pillow(j, what):
    mine, theirs = ljs.decode(j), pil_decode(j)
    assert mine.shape == theirs.shape
    d = np.abs(mine.astype(int) - theirs)
    assert not d.any(), "%s: %d bytes differ, by up to %d" % (what, int((d > 0).sum()), int(d.max()))


@pytest.mark.parametrize("w,h", SIZES)
def test_samplings_ref_is_what_pillow_decodes(w, h):
    """the yardstick: numpy restatement == Pillow's libjpeg-turbo, byte for byte, on every size x quality x source (uniform noise, 0 / 255 noise) x
    sampling and stream kind (restart intervals in MCUs -- blocks for gray --, optimised Huffman tables)"""
    rng = np.random.default_rng(1000 * w + h)
    for q in QUALITIES:
        for si, f in enumerate((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.where(rng.random((h, w, 1)) < .5, 0, 255).astype(np.uint8).repeat(3, 2))):
            for vi, (samp, kw) in enumerate(VARIANTS):
                _assert_ref_is_pillow(enc(f, q, samp, **kw), "%dx%d q%d source %d variant %d" % (w, h, q, si, vi))


@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_ref_is_what_pillow_decodes_1920_wide(name, samp):
    _assert_ref_is_pillow(enc(texture(1920, 24, seed=samp), 90, samp), "1920x24 " + name)


def test_samplings_ref_gray_ignores_its_sampling_factors():
    """T.81 A.2.2: a one-component scan is not interleaved, so the factors of the frame header mean nothing -- Pillow decodes the frame that says 0x22
    like the one that says 0x11, and so does the restatement"""
    j = enc(texture(21, 19, seed=2), 80, GRAY)
    i = j.index(b"\xff\xc0")
    assert j[i + 9] == 1 and j[i + 11] == 0x11
    j22 = j[:i + 11] + b"\x22" + j[i + 12:]
    assert np.array_equal(pil_decode(j22), pil_decode(j)) and np.array_equal(ljs.decode(j22), pil_decode(j))


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------------
SMALL = [(64, 48, 75), (100, 70, 95), (33, 21, 50), (16, 16, 100), (17, 9, 30), (1, 1, 75), (130, 34, 100), (3, 5, 75), (4, 7, 90), (31, 33, 60)]
# widths 1, 2, 4, 5, 6, 8 (4:2:2: chroma planes of 1, 2, 3 samples -- libjpeg replicates below 3, so the switch sits between w = 4 and w = 5), odd widths
# (the last output column is an even one), heights 1, 9, 31, and rows wider than one workgroup's MCUs (4:2:2: 16 MCUs = 256 pixels, 4:4:4 / gray: 32 MCUs
# = 256 pixels) with a partly filled last wave
NARROW = [(1, 1, 75), (2, 2, 75), (4, 4, 50), (5, 3, 95), (6, 2, 75), (5, 1, 90), (8, 1, 75), (1, 9, 75), (2, 31, 30), (4, 9, 85), (5, 9, 85), (7, 31, 100),
          (47, 15, 1), (18, 18, 10), (290, 20, 80), (337, 17, 92)]


def _batch(w, h, q, samp):
    """every kind of stream Pillow writes, two sets of quantiser tables in one call"""
    f = texture(w, h, seed=w + h)
    f2 = texture(w, h, seed=w + h + 5)
    plain = enc(f, q, samp)
    return [plain, enc(f, q, samp, optimize=True), enc(f, q, samp, restart_marker_blocks=3), enc(f, q, samp, restart_marker_rows=1), _strip_dht(plain),
            enc(f2, max(1, q - 20), samp)]


def _decode_and_compare(lvm, lib, alloc, read, cases, samp, ref=True, batch=_batch):
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
        ctx.mjpeg_set_samplings(samp)
        for (w, h, q) in cases:
            js = batch(w, h, q, samp)
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
                    assert np.array_equal(mine, ljs.decode(j)), "%dx%d q%d stream %d against libjpeg_ref_samplings" % (w, h, q, k)
                assert (got[k, :, w * 3:] == 0xEE).all(), "%dx%d q%d stream %d: padding bytes written" % (w, h, q, k)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_emu_byte_identical_to_pillow(lvm, emu, name, samp):
    _decode_and_compare(lvm, emu, *_numpy_alloc(), SMALL, samp)


@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_emu_narrow_and_ragged_sizes(lvm, emu, name, samp):
    _decode_and_compare(lvm, emu, *_numpy_alloc(), NARROW, samp)


@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_emu_long_streams_without_restart_markers(lvm, emu, name, samp):
    """streams of more than 2048 bytes without restart markers: what the default mode sends through the self-synchronising kernels"""
    def batch(w, h, q, samp):
        js = [enc(texture(w, h, seed=k), q, samp) for k in range(2)] + [enc(texture(w, h, seed=3), q, samp, optimize=True)]
        for j in js:
            hd = mo.parse_header(j)
            assert hd["restart"] == 0 and len(j) - hd["data_start"] > 2048 + 2
        return js
    _decode_and_compare(lvm, emu, *_numpy_alloc(), [(160, 96, 97), (130, 34, 100)], samp, batch=batch)


# ---- the second chunk of the chunked scans ---------------------------------------------------------------------------------------------------------------
# k_mjp_scan and k_mjp_dc scan 1024 values at a time with a carry: a frame reaches their second chunk with more than 1024 subsequences of 1024 bits and more
# than 1024 blocks of a component.  384 x 256 of uniform noise at quality 100 has 1536 luminance blocks in every sampling and 1198 (gray) .. 3136 (4:4:4)
# subsequences with libjpeg-turbo's tables; the batch asserts both from the stream it got, so that another encoder cannot make the case vacuous.
ALL4 = (("4:2:0", S420),) + NEW
SECOND_CHUNK = (384, 256, 100)


@functools.lru_cache(maxsize=None)
def _second_chunk_batch(w, h, q, samp):
    j = enc(np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8), q, samp)
    hd = mo.parse_header(j)
    assert hd["restart"] == 0 and j[-2:] == b"\xff\xd9"
    data = j[hd["data_start"]:-2]
    bits = 8 * (len(data) - data.count(b"\xff\x00"))
    hs, vs = hd["comps"][0][1:3] if len(hd["comps"]) == 3 else (1, 1)          # (a one-component scan is not interleaved: its factors mean nothing)
    yblocks = -(-w // (8 * hs)) * -(-h // (8 * vs)) * hs * vs
    assert bits > 1024 * 1024 and yblocks > 1024, (bits, yblocks)
    return [j, j]


@functools.lru_cache(maxsize=None)
def _oracle_frame(j):
    return mo.decode_frame(j)


def _second_chunk(lvm, lib, alloc, read, samp):
    """byte-identical to Pillow under the libjpeg kind (the numpy entropy decoder would take too long here: Pillow alone is the reference); 4:2:0 also
    under the replicating kind, bit-identical to the oracle's decode_frame"""
    _decode_and_compare(lvm, lib, alloc, read, [SECOND_CHUNK], samp, ref=False, batch=_second_chunk_batch)
    if samp != S420:
        return
    w, h, q = SECOND_CHUNK
    js = _second_chunk_batch(w, h, q, samp)
    want = _oracle_frame(js[0])
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_decoder(REPLICATE)
        buf = alloc(len(js), h, w * 3)
        ctx.mjpeg_decode_device(js, w, h, buf[0], stride=w * 3, frame_stride=w * 3 * h)
        got = read(buf)
        for k in range(len(js)):
            assert np.array_equal(got[k].reshape(h, w, 3), want), "replicating kind, stream %d against the oracle" % k
    finally:
        ctx.close()


@pytest.mark.parametrize("name,samp", ALL4)
def test_samplings_emu_second_chunk_of_the_scans(lvm, emu, name, samp):
    _second_chunk(lvm, emu, *_numpy_alloc(), samp)


def test_samplings_emu_both_entropy_paths():
    """as tests/test_mjpeg_decode_libjpeg.py: this file again with every frame without restart markers sent through the self-synchronising kernels
    (LVM_MJD_PARALLEL=2) and none (=0) -- the switch is read once per process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode in ("2", "0"):
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "tests/test_mjpeg_decode_samplings.py", "-m", "not gpu", "-k", "emu and not both_entropy_paths"],
                           capture_output=True, text=True, env=dict(os.environ, LVM_MJD_PARALLEL=mode), cwd=root, timeout=900)
        assert r.returncode == 0 and "passed" in r.stdout, (mode, (r.stdout + r.stderr)[-3000:])


def test_samplings_emu_the_switch(lvm, emu):
    ctx = lvm.Context(0, 1, emu)
    try:
        w, h = 66, 38
        f = texture(w, h, seed=9)
        out = np.zeros((2, h, w, 3), np.uint8)
        p = ctypes.c_void_p(out.ctypes.data)
        j420 = [mo.encode_frame(f, 85), enc(f, 85, S420)]
        new = {samp: enc(f, 85, samp) for _, samp in NEW}

        def run(js):
            out[...] = 0
            ctx.mjpeg_decode_device(js, w, h, p)
            return out[:len(js)].copy()

        def refused(js, why):
            with pytest.raises(lvm.LvmError, match=why) as e:
                ctx.mjpeg_decode_device(js, w, h, p)
            assert "lvm_mjpeg_decode: frame " in str(e.value)
        # the default mask: today's refusals, today's messages, under both kinds
        was = {}
        for kind in (REPLICATE, LIBJPEG):
            ctx.mjpeg_set_decoder(kind)
            was[kind] = run(j420)
            refused([new[S422]], "frame 0: sampling is not 4:2:0")
            refused([new[S444]], "frame 0: sampling is not 4:2:0")
            refused([new[GRAY]], "frame 0: not 8-bit three-component")
            refused([j420[1], new[S444]], "frame 1: sampling is not 4:2:0")
        assert all(np.array_equal(was[REPLICATE][k], mo.decode_frame(j)) and np.array_equal(was[LIBJPEG][k], pil_decode(j)) for k, j in enumerate(j420))
        # a bad mask is refused and changes nothing
        for bad in (0, 16, 31, -1):
            with pytest.raises(lvm.LvmError, match="lvm_mjpeg_set_samplings"):
                ctx.mjpeg_set_samplings(bad)
        refused([new[S422]], "sampling is not 4:2:0")
        # the mask set: they decode under the libjpeg kind; 4:2:0 is what it was under either kind
        ctx.mjpeg_set_samplings(ALL)
        for samp, j in new.items():
            assert np.array_equal(run([j, j])[1], pil_decode(j))
        assert np.array_equal(run(j420), was[LIBJPEG])
        for bad in (0, 16):
            with pytest.raises(lvm.LvmError, match="lvm_mjpeg_set_samplings"):
                ctx.mjpeg_set_samplings(bad)
        assert np.array_equal(run([new[GRAY]])[0], pil_decode(new[GRAY]))                 # (the refused masks changed nothing)
        # one sampling per call
        refused([new[S422], new[S444]], "frame 1: sampling differs from frame 0's")
        refused([j420[1], j420[1], new[GRAY]], "frame 2: sampling differs from frame 0's")
        # the replicating kind has no arithmetic for them; 4:2:0 under it is untouched
        ctx.mjpeg_set_decoder(REPLICATE)
        for name, samp in NEW:
            refused([new[samp]], "frame 0: %s needs LVM_MJPEG_DECODER_LIBJPEG" % name)
        assert np.array_equal(run(j420), was[REPLICATE])
        ctx.mjpeg_set_decoder(LIBJPEG)
        # a partial mask; what no mask allows: 4:4:0 (a 4:2:2 frame patched to 1 x 2), 4:1:1, four components
        ctx.mjpeg_set_samplings(S420 | S422)
        refused([new[S444]], "frame 0: sampling is not in the mask")
        refused([new[GRAY]], "frame 0: not 8-bit three-component")
        assert np.array_equal(run([new[S422]])[0], pil_decode(new[S422]))
        ctx.mjpeg_set_samplings(ALL)
        i = new[S422].index(b"\xff\xc0")
        assert new[S422][i + 11] == 0x21
        for factors in (0x12, 0x41):
            refused([new[S422][:i + 11] + bytes([factors]) + new[S422][i + 12:]], "frame 0: sampling is none of")
        buf = io.BytesIO()
        PIL_Image.fromarray(f).convert("CMYK").save(buf, "JPEG", quality=80)
        refused([buf.getvalue()], "frame 0: not 8-bit three-component")
        # a scan that names the components in another order than the frame header
        j = bytearray(new[S444])
        s = j.index(b"\xff\xda")
        j[s + 5], j[s + 7] = j[s + 7], j[s + 5]
        refused([bytes(j)], "frame 0: scan component order")
        # a gray frame whose header says 0x22 decodes like the one that says 0x11
        g = new[GRAY]
        i = g.index(b"\xff\xc0")
        assert np.array_equal(run([g[:i + 11] + b"\x22" + g[i + 12:]])[0], pil_decode(g))
        # back to the default mask: the refusals are back, 4:2:0 is what it was
        ctx.mjpeg_set_samplings(S420)
        refused([new[S422]], "frame 0: sampling is not 4:2:0")
        assert np.array_equal(run(j420), was[LIBJPEG])
    finally:
        ctx.close()


@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_emu_survives_corrupted_streams(lvm, emu, name, samp):
    """the damage of tests/test_mjpeg_decode_libjpeg.py::test_libjpeg_kind_emu_survives_corrupted_streams on the streams of one sampling: the call decodes
    something or fails with a message, and the context decodes the intact streams exactly afterwards (tools/emu_asan.sh and tools/emu_ubsan.sh run this
    file under the sanitizers: the parser and the coefficient layout of the MCU are what they check)"""
    rng = np.random.default_rng(3)
    f = texture(96, 64)
    streams = [enc(f, 85, samp), enc(f, 85, samp, restart_marker_blocks=2), enc(f, 97, samp, optimize=True)]
    ctx = lvm.Context(0, 1, emu)
    try:
        ctx.mjpeg_set_decoder(LIBJPEG)
        ctx.mjpeg_set_samplings(ALL)
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
        big = bytearray(streams[0])                                  # the largest quantisers: |coef * q| stays defined, whatever it decodes to
        i = big.index(b"\xff\xdb")
        big[i + 5:i + 5 + 64] = bytes([255] * 64)
        ctx.mjpeg_decode_device([bytes(big)], 96, 64, p)
        for j in streams:
            ctx.mjpeg_decode_device([j], 96, 64, p)
            assert np.array_equal(out[0].reshape(64, 96, 3), pil_decode(j))
    finally:
        ctx.close()


def _transcode_case(lvm, lib, samp, w, h, n, split, q_in, q_out):
    """lvm_export_mjpeg_frames on frames of the sampling == lvm_export_frames_mjpeg fed with Pillow's decoded frames, byte for byte"""
    from helpers import c_params
    ck, pk = lvm.synth.config(0)                                     # Laplace
    clip = lvm.synth.Clip(seed=7, **dict(ck, w=w, h=h))
    jin = [enc(clip.frame(t), q_in, samp, **(dict(optimize=True) if t % 2 else {})) for t in range(n)]
    decoded = [pil_decode(j) for j in jin]
    pre = lvm.LvmPreprocessParams(1, 0, 0.0, 0.0, 1.0, 1.0, 0)
    cp = c_params(lvm, pk)
    a, b = lvm.Context(0, 1, lib), lvm.Context(0, 1, lib)
    try:
        b.mjpeg_set_decoder(LIBJPEG)
        b.mjpeg_set_samplings(samp)
        want, prod_a = a.export_frames_mjpeg(decoded, pre, cp, split, quality=q_out)
        got, prod_b = b.export_mjpeg_frames(jin, w, h, pre, cp, split, quality=q_out)
        assert list(prod_a) == list(prod_b) and len(got) == len(want) == n
        for k in range(n):
            assert got[k] == want[k], "frame %d" % k
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name,samp", [("4:2:2", S422), ("gray", GRAY)])
def test_samplings_emu_export_mjpeg_to_mjpeg(lvm, emu, name, samp):
    _transcode_case(lvm, emu, samp, 80, 60, 5, 1, 85, 80)


# ---- the host shims carry the mask -----------------------------------------------------------------------------------------------------------------------
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
int main(int argc, char** argv) {       // JPEG frame, output path, w, h
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<std::uint8_t> j(1 << 20);
    j.resize(std::fread(j.data(), 1, j.size(), f));
    std::fclose(f);
    lvm::MjpegAviReader plain, rd(LVM_MJPEG_DECODER_LIBJPEG, LVM_MJPEG_SAMPLING_ALL);
    if (plain.samplings() != LVM_MJPEG_SAMPLING_420 || rd.samplings() != LVM_MJPEG_SAMPLING_ALL || rd.decoder() != LVM_MJPEG_DECODER_LIBJPEG) return 3;
    plain.set_samplings(LVM_MJPEG_SAMPLING_422);
    if (plain.samplings() != LVM_MJPEG_SAMPLING_422) return 4;
    lvm::ExportRunner<Traits> runner(0, 4);
    int refused = 0;
    for (unsigned bad : {0u, 16u}) { try { runner.set_mjpeg_samplings(bad); } catch (const lvm::Error& e) { refused += e.status() == LVM_ERR_INVALID; } }
    if (refused != 2) return 5;
    runner.set_mjpeg_decoder(rd.decoder());
    void* out = nullptr;                    // (page-locked host memory: device-accessible on the GPU, plain memory in the emulation build)
    if (lvm_host_alloc((size_t)w * h * 3, &out) != LVM_OK) return 6;
    const size_t offs[2] = {0, j.size()};
    if (lvm_mjpeg_decode_device(runner.handle(), j.data(), offs, 1, w, h, (std::uint8_t*)out, (std::ptrdiff_t)w * 3, (std::ptrdiff_t)w * 3 * h) != LVM_ERR_INVALID) return 7;   // the default mask
    runner.set_mjpeg_samplings(rd.samplings());
    if (lvm_mjpeg_decode_device(runner.handle(), j.data(), offs, 1, w, h, (std::uint8_t*)out, (std::ptrdiff_t)w * 3, (std::ptrdiff_t)w * 3 * h) != LVM_OK) {
        std::printf("%s\n", lvm_last_error(runner.handle()));
        return 8;
    }
    std::FILE* o = std::fopen(argv[2], "wb");
    const bool ok = o && std::fwrite(out, 1, (size_t)w * h * 3, o) == (size_t)w * h * 3 && std::fclose(o) == 0;
    lvm_host_free(out);
    return ok ? 0 : 9;
}
"""


def test_samplings_emu_through_the_host_shims(tmp_path, emu):
    """host/HipMjpegWriter.hpp's reader carries the mask next to the decoder kind, host/HipExportRunner.hpp applies it to its context
    (lvm::Magnifier::mjpeg_set_samplings): a 4:2:2 frame is refused before and is Pillow's frame after; a bad mask throws lvm::Error"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    w, h = 50, 34
    j = enc(texture(w, h, seed=4), 88, S422)
    (tmp_path / "frame.jpg").write_bytes(j)
    (tmp_path / "t.cpp").write_text(SHIM_SRC)
    libdir = os.path.join(root, "tests", "emu", "_build")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", str(tmp_path / "t.cpp"), "-I", os.path.join(root, "include"),
                           "-I", os.path.join(root, "live-video-magnification_amd", "host"), "-L", libdir, "-llvm_emu", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "t")])
    r = subprocess.run([str(tmp_path / "t"), str(tmp_path / "frame.jpg"), str(tmp_path / "out.bin"), str(w), str(h)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout + r.stderr)
    assert np.array_equal(np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8).reshape(h, w, 3), pil_decode(j))


# ---- the GPU -------------------------------------------------------------------------------------------------------------------------------------------
def _torch_alloc():
    import torch

    def alloc(n, h, row):
        t = torch.full((n, h, row), 0xEE, dtype=torch.uint8, device="cuda")
        return (ctypes.c_void_p(t.data_ptr()), t)
    return alloc, (lambda b: b[1].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_gpu_byte_identical_to_pillow(lvm, hip, name, samp):
    _decode_and_compare(lvm, hip, *_torch_alloc(), SMALL + NARROW, samp)


@pytest.mark.gpu
@pytest.mark.parametrize("name,samp", NEW)
def test_samplings_gpu_322x182_and_1920_wide(lvm, hip, name, samp):
    """322 x 182 at quality 90 without restart markers (the self-synchronising kernels) and with restart intervals of 8 blocks (a lane per interval), and a
    strip as wide as 1080p: every byte is Pillow's (the numpy entropy decoder would take minutes at these sizes: Pillow alone is the reference)"""
    def batch(w, h, q, samp):
        f, f2 = texture(w, h, seed=w + h), texture(w, h, seed=w + h + 5)
        js = [enc(f, q, samp), enc(f2, q, samp, optimize=True), enc(f, q, samp, restart_marker_blocks=8), enc(f2, q, samp, restart_marker_blocks=8)]
        if w == 322:
            assert mo.parse_header(js[0])["restart"] == 0 and len(js[0]) > 2048 and mo.parse_header(js[2])["restart"] == 8
        return js
    _decode_and_compare(lvm, hip, *_torch_alloc(), [(322, 182, 90), (1920, 24, 90)], samp, ref=False, batch=batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,samp", ALL4)
def test_samplings_gpu_second_chunk_of_the_scans(lvm, hip, name, samp):
    _second_chunk(lvm, hip, *_torch_alloc(), samp)


@pytest.mark.gpu
def test_samplings_gpu_export_mjpeg_to_mjpeg(lvm, hip):
    _transcode_case(lvm, hip, S422, 322, 182, 5, 1, 90, 85)


@pytest.mark.gpu
def test_samplings_gpu_riesz_end_to_end(lvm, hip):
    """a Riesz magnification of 6 frames of a 4:2:2 source decoded on the device == the one fed by Pillow's frames on a second context, byte for byte"""
    import torch
    from helpers import c_params
    w, h, n = 320, 180, 6
    ck, pk = lvm.synth.config(2, (w, h, 5))
    clip = lvm.synth.Clip(**ck)
    cp = c_params(lvm, pk)
    js = [enc(clip.frame(t), 90, S422) for t in range(n)]
    fb = w * h * 3
    st = torch.cuda.current_stream().cuda_stream
    a, b = lvm.Context(0, 1, hip), lvm.Context(0, 1, hip)
    try:
        a.mjpeg_set_decoder(lvm.MJPEG_DECODER_LIBJPEG)
        a.mjpeg_set_samplings(lvm.MJPEG_SAMPLING_422)
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
        assert torch.equal(d_out, u_out), "the magnified frames differ"
    finally:
        a.close()
        b.close()
