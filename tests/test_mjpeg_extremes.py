"""Motion-JPEG at the ends of its tables and limits (csrc/mjpeg.hip, csrc/mjpeg_decode.hip): the content of tests/test_mjpeg*.py -- a sine texture plus noise --
stops at AC category 9 (10 on the GPU), DC difference category 10 and 920 restart intervals per frame, and no call there has more than three frames.

Here: frames designed to reach the longest and the shortest code words (tests/jpeg_content.py: DC differences of category 11 in both tables, AC coefficients
of category 10 in both tables -- the 26-bit words `put_bits` and MJ_BLOCK_WORDS are dimensioned for --, ZRL symbols, blocks without end-of-block, blocks of four
bits), more than 1024 intervals per frame (the second chunk of k_mj_frame_offsets and its 64-bit carry), the 512-MCU clamp of an interval, the widest and the
tallest frame and the refusal beyond them, calls of 19 frames (sub-calls of 8 with the download running beside them) and a capacity overflow in the middle of
a call.  Every comparison is byte equality with oracle/mjpeg_oracle.py (the decoder's libjpeg kind: with Pillow); the same bodies run on the emulation build
and, marked gpu, through the C ABI on the device.  What a frame reaches is asserted on the ORACLE first (jpeg_content.coverage), so that a change of the
content cannot silently stop reaching the symbols."""
import ctypes
import functools

import numpy as np
import pytest

import jpeg_content as jc
from oracle import mjpeg_oracle as mo
from test_mjpeg import _numpy_dev, decode
from test_mjpeg_decode import _numpy_alloc, pil_encode

FRAMES = {"basis": jc.basis, "chroma": jc.chroma, "flat": jc.flat}
QUALITIES = (100, 50, 1)
RESTARTS = (0, 1, 3)                                     # 0: the default of 8 MCUs
SAME_SIZE = (128, 64)                                    # the three designed frames padded to one size, for calls of three frames
TILED = {"basis_tiled": "basis", "chroma_tiled": "chroma"}      # 2 x 2 times the frame: libjpeg's streams of these are long enough for the self-synchronising kernels
MJP_FROM_BYTES = 2048                                    # csrc/mjpeg_decode.hip: a frame without DRI and this much entropy data goes to the k_mjp_* kernels


@functools.lru_cache(maxsize=None)
def frame(name):
    f = jc.tiled(frame(TILED[name])) if name in TILED else FRAMES[name]()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def frame_same_size(name):
    f = jc.padded(frame(name), *SAME_SIZE)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def noise(w, h, seed):
    f = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle_stream(kind, name, quality, restart):
    """the oracle's stream, computed once for the emulation and the GPU test"""
    f = {"designed": frame, "same_size": frame_same_size}[kind](name) if isinstance(name, str) else noise(*name)
    return mo.encode_frame(f, quality, restart=restart)


def _torch_dev():
    import torch

    def to_dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return (ctypes.c_void_p(t.data_ptr()), t)
    return to_dev


def _torch_alloc():
    import torch

    def alloc(n, h, row):
        t = torch.full((n, h, row), 0xEE, dtype=torch.uint8, device="cuda")
        return (ctypes.c_void_p(t.data_ptr()), t)
    return alloc, (lambda b: b[1].cpu().numpy())


def _stage(frames, pad):
    """[n][h][w][3] -> [n][h][w * 3 + pad] with 0xEE behind every row"""
    n, h, w, _ = frames.shape
    staged = np.full((n, h, w * 3 + pad), 0xEE, np.uint8)
    staged[:, :, :w * 3] = frames.reshape(n, h, w * 3)
    return staged


def _encode(ctx, to_dev, frames, quality, pad=0, capacity=None):
    """lvm_mjpeg_encode_device on [n][h][w][3] frames staged with `pad` bytes behind every row -> (frames as bytes, offsets[0..n])"""
    n, h, w, _ = frames.shape
    d = to_dev(_stage(frames, pad))
    row = w * 3 + pad
    cap = int(ctx.lib.lvm_mjpeg_bound(w, h)) * n if capacity is None else int(capacity)
    out = np.full(cap, 0xA5, np.uint8)
    offs = (ctypes.c_size_t * (n + 1))()
    ctx._check(ctx.lib.lvm_mjpeg_encode_device(ctx.h, d[0], w, h, row, row * h, n, int(quality), out.ctypes.data, cap, offs))
    offs = [int(o) for o in offs]
    return [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)], offs


def _same(got, want, what):
    assert got == want, "%s: %d vs %d bytes, first difference at %d" % (
        what, len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))


def _check_call(got, offs, want, what):
    """every frame the oracle's, and the offsets are the running sum of the frame lengths"""
    assert offs[0] == 0 and len(got) == len(want)
    for k, (g, w_) in enumerate(zip(got, want)):
        assert offs[k + 1] - offs[k] == len(w_), "%s: frame %d is %d bytes long by the offsets, %d in the oracle" % (what, k, offs[k + 1] - offs[k], len(w_))
        _same(g, w_, "%s, frame %d" % (what, k))


# ---- 1. the designed frames reach what they were designed for (the oracle alone) ----------------------------------------------------------------------------

def test_designed_frames_reach_the_ends_of_the_tables():
    b = jc.coverage(frame("basis"), 100, 1)
    assert b["ac_cat"][0] == 10 and b["ac_max"][0] == 1020 and b["dc_cat"][0] == 11 and b["zrl"] >= 20 and b["no_eob"] >= 1
    for restart in RESTARTS:
        assert jc.coverage(frame("basis"), 100, restart)["dc_cat"][0] == 11
    per_restart = [jc.coverage(frame("chroma"), 100, r) for r in RESTARTS]
    for c in per_restart:
        assert c["ac_cat"][1] == 10 and c["ac_max"][1] == 1020 and c["dc_cat"] == (11, 11) and c["zrl"] >= 15 and c["no_eob"] >= 1 and c["ff00"] >= 1
    assert max(c["ff_at_marker"] for c in per_restart) >= 1                              # a stuffed FF directly in front of a marker
    for name in ("basis", "chroma"):
        for restart in RESTARTS:
            low = jc.coverage(frame(name), 1, restart)
            assert low["zrl"] >= 20 and max(low["ac_cat"]) <= 4 and max(low["dc_cat"]) <= 4, (name, restart, low)
        c = jc.coverage(frame_same_size(name), 100, 0)                                   # the padded forms keep the long words
        assert c["ac_cat"][0] == 10 and c["dc_cat"][0] == 11
    assert jc.coverage(frame_same_size("chroma"), 100, 0)["ac_cat"][1] == 10 and jc.coverage(frame_same_size("chroma"), 100, 0)["dc_cat"][1] == 11
    t = jc.coverage(frame("basis_tiled"), 100, 0)                                        # the tiled forms (the decoder's self-synchronising path) likewise
    assert t["ac_cat"][0] == 10 and t["dc_cat"][0] == 11 and t["zrl"] >= 80 and t["no_eob"] >= 4
    t = jc.coverage(frame("chroma_tiled"), 100, 0)
    assert t["ac_cat"] == (10, 10) and t["dc_cat"] == (11, 11) and t["zrl"] >= 60 and t["no_eob"] >= 4
    t = jc.coverage(frame("basis_tiled"), 1, 0)
    assert t["zrl"] >= 80 and max(t["ac_cat"]) <= 4 and max(t["dc_cat"]) <= 4
    f = jc.coverage(frame("flat"), 50, 3)
    assert f["ac_cat"] == (0, 0) and f["zrl"] == 0 and f["no_eob"] == 0 and f["intervals"] == 4      # 4 x 3 MCUs in threes
    # the shortest blocks: 12 MCUs of 6 blocks in at most 6 bits each (T.81 K.3: DC category 0 is 2 bits, end-of-block 2 or 4)
    assert len(oracle_stream("designed", "flat", 50, 1000)) - len(mo.header(56, 40, 50, 512)) - 2 <= (12 * 6 * 6 + 10 + 7) // 8


def test_coverage_counts_what_the_stream_holds():
    """every counter against the stream itself: the coefficients mo.decode_coefficients reads out of mo.encode_frame's bytes (categories, zero runs and DC
    differences worked out a second way, with whole-array operations), its DRI, its markers and its stuffed bytes"""
    for name, q, restart in (("basis", 100, 1), ("chroma", 100, 3), ("chroma", 1, 0), ("basis_tiled", 1, 0), ("flat", 50, 3)):
        f = frame(name)
        c = jc.coverage(f, q, restart)
        j = oracle_stream("designed", name, q, restart)
        hd, coef = mo.decode_coefficients(j)
        assert np.array_equal(coef, mo.coefficients(f, q))
        ac_max = (int(np.abs(coef[:, :, :4, 1:]).max()), int(np.abs(coef[:, :, 4:, 1:]).max()))
        assert c["ac_max"] == ac_max and c["ac_cat"] == tuple(v.bit_length() for v in ac_max)
        assert c["no_eob"] == int((coef[..., 63] != 0).sum())
        # ZRL symbols: a non-zero AC coefficient at k whose previous non-zero AC coefficient is at p (0: none) is preceded by (k - p - 1) // 16 of them
        blocks = coef.reshape(-1, 64)
        k = np.arange(64)
        at = np.where(blocks != 0, k, 0)
        at[:, 0] = 0
        before = np.maximum.accumulate(at, axis=1)[:, :-1]
        assert c["zrl"] == int((((k[1:] - before - 1) // 16) * (blocks[:, 1:] != 0)).sum())
        # DC differences: per component in coding order, the predictor 0 at the start of every interval of hd["restart"] MCUs
        mcus = coef.reshape(-1, 6, 64)
        dc = [0, 0]
        for m0 in range(0, len(mcus), hd["restart"]):
            part = mcus[m0:m0 + hd["restart"], :, 0].astype(np.int64)
            for t, seq in ((0, part[:, :4].reshape(-1)), (1, part[:, 4]), (1, part[:, 5])):
                dc[t] = max(dc[t], int(np.abs(np.diff(seq, prepend=0)).max()).bit_length())
        assert c["dc_cat"] == tuple(dc)
        ivs = mo.split_intervals(j[hd["data_start"]:])
        assert c["intervals"] == len(ivs) and hd["restart"] == jc.interval_length(coef.shape[0] * coef.shape[1], restart)
        assert c["ff00"] == sum(iv.count(b"\xff\x00") for iv in ivs) and c["ff_at_marker"] == sum(iv.endswith(b"\xff\x00") for iv in ivs)


# ---- 2. the encoder -----------------------------------------------------------------------------------------------------------------------------------------

def _designed_frames(lvm, lib, to_dev, quality):
    ctx = lvm.Context(0, 1, lib)
    try:
        for restart in RESTARTS:
            ctx.mjpeg_set_restart_interval(restart)
            for name in FRAMES:
                f = frame(name)
                got, offs = _encode(ctx, to_dev, f[None], quality, pad=5 if name != "flat" else 3)
                _check_call(got, offs, [oracle_stream("designed", name, quality, restart)], "%s q%d restart %d" % (name, quality, restart))
                assert decode(got[0]).shape == f.shape
            names = list(FRAMES)
            got, offs = _encode(ctx, to_dev, np.stack([frame_same_size(n) for n in names]), quality, pad=7)
            _check_call(got, offs, [oracle_stream("same_size", n, quality, restart) for n in names], "three frames q%d restart %d" % (quality, restart))
            for g in got:
                assert decode(g).shape == (SAME_SIZE[1], SAME_SIZE[0], 3)
    finally:
        ctx.close()


@pytest.mark.parametrize("quality", QUALITIES)
def test_extremes_emu_designed_frames(lvm, emu, quality):
    """basis / chroma / flat x restart (8, 1, 3) at one quality, each alone with ragged rows and the three, padded to one size, in one call"""
    _designed_frames(lvm, emu, _numpy_dev(), quality)


@pytest.mark.gpu
@pytest.mark.parametrize("quality", QUALITIES)
def test_extremes_gpu_designed_frames(lvm, hip, quality):
    _designed_frames(lvm, hip, _torch_dev(), quality)


def _more_than_1024_intervals(lvm, lib, to_dev):
    """528 x 512 = 33 x 32 MCUs at one MCU per interval: k_mj_frame_offsets walks a second chunk, its carry is the offset of interval 1024"""
    w, h, q = 528, 512, 50
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_restart_interval(1)
        got, offs = _encode(ctx, to_dev, noise(w, h, 1)[None], q)
    finally:
        ctx.close()
    hd = mo.parse_header(got[0])
    nint = -(-(((hd["w"] + 15) // 16) * ((hd["h"] + 15) // 16)) // hd["restart"])
    assert (hd["w"], hd["h"], hd["restart"]) == (w, h, 1) and nint == 1056 and nint > 1024
    _check_call(got, offs, [oracle_stream("noise", (w, h, 1), q, 1)], "528 x 512, 1056 intervals")
    assert decode(got[0]).shape == (h, w, 3)


def test_extremes_emu_more_than_1024_intervals(lvm, emu):
    _more_than_1024_intervals(lvm, emu, _numpy_dev())


@pytest.mark.gpu
def test_extremes_gpu_more_than_1024_intervals(lvm, hip):
    _more_than_1024_intervals(lvm, hip, _torch_dev())


def _interval_clamp(lvm, lib, to_dev):
    """1000 MCUs per interval asked for, 512 given (MJ_MAX_MW, k_mj_scan's LDS): 528 MCUs are an interval of 512 and one of 16"""
    w, h, q = 528, 256, 50
    f = noise(w, h, 2)
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_restart_interval(1000)
        got, offs = _encode(ctx, to_dev, f[None], q, pad=4)
    finally:
        ctx.close()
    hd = mo.parse_header(got[0])
    assert hd["restart"] == 512
    ivs = mo.split_intervals(got[0][hd["data_start"]:])
    mcus = mo.coefficients(f, q).reshape(528, 6, 64)
    tabs = tuple(mo.huff_codes(s) for s in (mo.DC_LUMA, mo.AC_LUMA, mo.DC_CHROMA, mo.AC_CHROMA))
    assert len(ivs) == 2
    _same(ivs[0], mo.entropy_interval(mcus[:512], tabs), "the interval of 512 MCUs")
    _same(ivs[1], mo.entropy_interval(mcus[512:], tabs), "the interval of 16 MCUs")
    _check_call(got, offs, [oracle_stream("noise", (w, h, 2), q, 1000)], "528 x 256, restart 1000")


def test_extremes_emu_interval_clamp(lvm, emu):
    _interval_clamp(lvm, emu, _numpy_dev())


@pytest.mark.gpu
def test_extremes_gpu_interval_clamp(lvm, hip):
    _interval_clamp(lvm, hip, _torch_dev())


SIZE_LIMITS = [(8192, 16, 1000), (8192, 16, 1), (16, 4100, 0)]          # a full 512-MCU interval in one MCU row; 512 intervals; 257 MCU rows


def _size_limit(lvm, lib, to_dev, w, h, restart):
    q = 60
    ctx = lvm.Context(0, 1, lib)
    try:
        ctx.mjpeg_set_restart_interval(restart)
        got, offs = _encode(ctx, to_dev, noise(w, h, 3)[None], q)
    finally:
        ctx.close()
    _check_call(got, offs, [oracle_stream("noise", (w, h, 3), q, restart)], "%d x %d restart %d" % (w, h, restart))
    assert decode(got[0]).shape == (h, w, 3)


@pytest.mark.parametrize("w,h,restart", SIZE_LIMITS)
def test_extremes_emu_size_limits(lvm, emu, w, h, restart):
    _size_limit(lvm, emu, _numpy_dev(), w, h, restart)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,restart", SIZE_LIMITS)
def test_extremes_gpu_size_limits(lvm, hip, w, h, restart):
    _size_limit(lvm, hip, _torch_dev(), w, h, restart)


def _size_refusals(lvm, lib, to_dev):
    ctx = lvm.Context(0, 1, lib)
    try:
        for (w, h) in ((8208, 16), (16, 16400)):
            with pytest.raises(lvm.LvmError, match="out of range"):
                _encode(ctx, to_dev, np.zeros((1, h, w, 3), np.uint8), 60)
        got, offs = _encode(ctx, to_dev, frame("chroma")[None], 100)
        _check_call(got, offs, [oracle_stream("designed", "chroma", 100, 0)], "after the refusals")
    finally:
        ctx.close()


def test_extremes_emu_size_refusals(lvm, emu):
    _size_refusals(lvm, emu, _numpy_dev())


@pytest.mark.gpu
def test_extremes_gpu_size_refusals(lvm, hip):
    _size_refusals(lvm, hip, _torch_dev())


def _long_sequences(lvm, lib, to_dev):
    """one context: 19 frames in one call (sub-calls of 8, 8 and 3: from the third on, finished frames are downloaded while later ones encode; frame0, the
    running byte count and the mirror of the offsets are carried from sub-call to sub-call), then 9 frames (8 + 1) at another interval length, then one at
    another quality"""
    w, h = 40, 24
    ctx = lvm.Context(0, 1, lib)
    try:
        for n, q, restart, seed0 in ((19, 90, 0, 100), (9, 90, 2, 200), (1, 35, 2, 300)):
            ctx.mjpeg_set_restart_interval(restart)
            frames = np.stack([noise(w, h, seed0 + k) for k in range(n)])
            got, offs = _encode(ctx, to_dev, frames, q, pad=2)
            _check_call(got, offs, [oracle_stream("noise", (w, h, seed0 + k), q, restart) for k in range(n)], "%d frames q%d restart %d" % (n, q, restart))
    finally:
        ctx.close()


def test_extremes_emu_long_sequences(lvm, emu):
    _long_sequences(lvm, emu, _numpy_dev())


@pytest.mark.gpu
def test_extremes_gpu_long_sequences(lvm, hip):
    _long_sequences(lvm, hip, _torch_dev())


def _capacity_overflow_in_a_sequence(lvm, lib, to_dev):
    """five 64 x 48 frames at quality 100, four of noise and a flat (small) one, and room for two noise frames and the flat one: the call fails with 'too small'
    whether the flat frame is the middle one (frames 0..2 fit exactly, 3 and 4 do not) or follows the first one that does not fit (by k_mj_offsets' rule frame 2
    is skipped, frame 3 fits into what is left and frame 4 does not; what a failed call leaves in the output is not part of the contract and not looked at) -- and
    the same context returns all five, byte for byte, once the capacity suffices.  The lengths are the oracle's."""
    w, h, q = 64, 48, 100
    small = np.full((h, w, 3), 7, np.uint8)
    ctx = lvm.Context(0, 1, lib)
    try:
        for flat_at in (2, 3):
            frames = np.stack([small if k == flat_at else noise(w, h, 400 + k) for k in range(5)])
            want = [mo.encode_frame(frames[k], q) if k == flat_at else oracle_stream("noise", (w, h, 400 + k), q, 0) for k in range(5)]
            assert len(want[flat_at]) < min(len(want[k]) for k in range(5) if k != flat_at) // 4
            cap = len(want[0]) + len(want[1]) + len(want[flat_at])
            with pytest.raises(lvm.LvmError, match="too small"):
                _encode(ctx, to_dev, frames, q, capacity=cap)
            got, offs = _encode(ctx, to_dev, frames, q, capacity=sum(len(j) for j in want))          # exactly enough
            _check_call(got, offs, want, "five frames, the flat one at %d" % flat_at)
    finally:
        ctx.close()


def test_extremes_emu_capacity_overflow_in_a_sequence(lvm, emu):
    _capacity_overflow_in_a_sequence(lvm, emu, _numpy_dev())


@pytest.mark.gpu
def test_extremes_gpu_capacity_overflow_in_a_sequence(lvm, hip):
    _capacity_overflow_in_a_sequence(lvm, hip, _torch_dev())


# ---- 3. the decoder on the same symbols ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def decoder_case(name, quality):
    """five streams of one designed frame and what the two kinds must make of each: (streams, mo.decode_frame of each, Pillow's decode of each)"""
    f = frame(name)
    js = [oracle_stream("designed", name, quality, 0), oracle_stream("designed", name, quality, 1), oracle_stream("designed", name, quality, 1000),
          pil_encode(f, quality, subsampling=2), pil_encode(f, quality, subsampling=2, optimize=True)]
    assert [mo.parse_header(j)["restart"] for j in js] == [8, 1, 512, 0, 0]
    assert len(mo.split_intervals(js[2][mo.parse_header(js[2])["data_start"]:])) == 1                # no marker in the data
    entropy_bytes = [len(j) - mo.parse_header(j)["data_start"] - 2 for j in js]                     # what the decoder's dispatch rule looks at
    if quality == 100:                                                                             # libjpeg's quantiser at 100 is all ones as well: the long words again
        for j in js[3:]:
            _, coef = mo.decode_coefficients(j)
            blocks = (0, 1, 2, 3) if name.startswith("basis") else (4, 5)
            assert int(np.abs(coef[:, :, blocks, 1:]).max()).bit_length() == 10
            dc = coef.reshape(-1, 6, 64)[:, :, 0].astype(np.int64)                                  # no DRI: one predictor chain per component over the whole frame
            chains = [dc[:, :4].reshape(-1)] if name.startswith("basis") else [dc[:, 4], dc[:, 5]]
            assert all(int(np.abs(np.diff(c, prepend=0)).max()).bit_length() == 11 for c in chains)
        # libjpeg's streams carry no DRI: the tiled frames' ones go to the self-synchronising kernels (k_mjp_*), the others' to one lane
        assert all(n >= MJP_FROM_BYTES for n in entropy_bytes[3:]) if name in TILED else all(n < MJP_FROM_BYTES for n in entropy_bytes[3:]), entropy_bytes
    if (name, quality) == ("basis_tiled", 1):                                                       # ZRL symbols with short words on that path
        assert entropy_bytes[3] >= MJP_FROM_BYTES
    return js, [mo.decode_frame(j) for j in js], [decode(j) for j in js]


def _decode_designed(lvm, lib, alloc, read):
    ctx = lvm.Context(0, 1, lib)
    try:
        for name in ("basis", "chroma", "basis_tiled", "chroma_tiled"):
            h, w, _ = frame(name).shape
            for q in QUALITIES:
                js, replicate, libjpeg = decoder_case(name, q)
                for kind, want in ((lvm.MJPEG_DECODER_REPLICATE, replicate), (lvm.MJPEG_DECODER_LIBJPEG, libjpeg)):
                    ctx.mjpeg_set_decoder(kind)
                    row = w * 3 + 5
                    buf = alloc(len(js), h, row)
                    ctx.mjpeg_decode_device(js, w, h, buf[0], stride=row, frame_stride=row * h)
                    got = read(buf)
                    for k in range(len(js)):
                        mine = got[k, :, :w * 3].reshape(h, w, 3)
                        d = np.abs(mine.astype(int) - want[k])
                        assert not d.any(), "%s q%d kind %d stream %d: %d bytes differ, by up to %d" % (name, q, kind, k, int((d > 0).sum()), int(d.max()))
                        assert (got[k, :, w * 3:] == 0xEE).all(), "%s q%d kind %d stream %d: padding bytes written" % (name, q, kind, k)
    finally:
        ctx.close()


def test_extremes_emu_decode_designed_frames(lvm, emu):
    """basis / chroma and their 2 x 2 tiled forms at quality 100, 50, 1 as the oracle writes them (intervals of 8, of 1, one interval without a marker) and as
    libjpeg does (no DRI; standard and optimised tables), five streams per call: the replicating kind == mo.decode_frame, the libjpeg kind == Pillow.
    Both entropy decoders see the long words in the same body: a stream with a DRI (the oracle's, also the one whose single interval holds the whole frame: DRI
    512) gets a lane per interval (k_mjd_huffman), so do libjpeg's streams of basis() and chroma(), which are shorter than 2 KB; libjpeg's streams of the tiled
    frames at quality 100 are longer and go through the self-synchronising kernels (k_mjp_*) -- decoder_case asserts which is which on the streams."""
    _decode_designed(lvm, emu, *_numpy_alloc())


@pytest.mark.gpu
def test_extremes_gpu_decode_designed_frames(lvm, hip):
    _decode_designed(lvm, hip, *_torch_alloc())


def _round_trip(lvm, lib, to_dev, alloc, read):
    """the device encoder's stream of chroma() at quality 100 through the device decoder == the oracle's decode of the oracle's stream"""
    f = frame("chroma")
    h, w, _ = f.shape
    ctx = lvm.Context(0, 1, lib)
    try:
        got, _ = _encode(ctx, to_dev, f[None], 100, pad=5)
        buf = alloc(1, h, w * 3 + 5)
        ctx.mjpeg_decode_device(got, w, h, buf[0], stride=w * 3 + 5, frame_stride=(w * 3 + 5) * h)
        out = read(buf)
    finally:
        ctx.close()
    assert np.array_equal(out[0, :, :w * 3].reshape(h, w, 3), decoder_case("chroma", 100)[1][0]) and (out[0, :, w * 3:] == 0xEE).all()


def test_extremes_emu_round_trip(lvm, emu):
    _round_trip(lvm, emu, _numpy_dev(), *_numpy_alloc())


@pytest.mark.gpu
def test_extremes_gpu_round_trip(lvm, hip):
    _round_trip(lvm, hip, _torch_dev(), *_torch_alloc())
