"""The memory layouts a caller may hand to lvm_process_device / lvm_process_device_frames: frames that are rectangles inside larger
buffers (a cv::Mat ROI, the export's ROI view of a decoded frame), in temporal batches, with every term of the launch code's
alignment tests made false on its own, and with the wave-strip kernels of the production sizes forced onto small frames -- where the
profile must show the kernel the launch code picks for that layout (parity_matrix.LAYOUT_LAUNCHES), so that no case passes on a fall-back
(tests/parity_matrix.py: LAYOUTS, LAYOUT_CASES, LAYOUT_FORCED; helpers.layout_clip).

  emulation build: every case, all three modes, the oracle's bytes bit for bit (the emulation's buffer resources are range-checked);
  gfx950 build   : Laplace and Color the oracle's bytes bit for bit (the claim of tests/test_gpu_exact.py for packed rows);
                   Riesz (device acosf / sinf / cosf) within the parity bars of the oracle AND byte-equal to a second context that
                   gets the same frames packed -- the arithmetic of the exact flavour does not depend on the kernel family;
  both           : no byte of the output allocation outside the rectangles is written.

Row strides that cannot hold their pixels are refused (LVM_ERR_INVALID) before any state changes: emulation build only, the host
code is the same translation unit and a GPU must never be handed such a layout."""
import numpy as np
import pytest

import parity_matrix as M
from helpers import HostMem, TorchMem, c_params

HOST = HostMem()


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---- emulation build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,w,h,levels,ns,name", M.LAYOUT_CASES, ids=_ids(M.LAYOUT_CASES))
def test_layout_emu_bit_exact(lvm, po, emu, idx, w, h, levels, ns, name):
    M.layout_case(lvm, po, emu, HOST, idx, w, h, levels, ns, name)


@pytest.mark.parametrize("force,name", M.LAYOUT_FORCED_CASES, ids=_ids(M.LAYOUT_FORCED_CASES))
def test_layout_emu_forced_strip_kernels_bit_exact(lvm, po, emu, force, name):
    M.layout_forced_case(lvm, po, emu, HOST, force, name)


# ---- the refusals (emulation build only) ------------------------------------------------------------------------------------------
W, H, LEVELS = 64, 48, 3
ROW, FB = W * 3, W * H * 3
# (n_streams, in_stride, in_stream_stride, out_stride, out_stream_stride, message)
REFUSED = [
    (1, ROW - 1, FB, ROW, FB, "frame stride too small"),
    (1, ROW, FB, ROW - 1, FB, "frame stride too small"),
    (1, 0, FB, ROW, FB, "frame stride too small"),
    (1, ROW, FB, 0, FB, "frame stride too small"),
    (1, -ROW, FB, ROW, FB, "frame stride too small"),
    (1, ROW, FB, -ROW, FB, "frame stride too small"),
    (2, ROW, FB, ROW, 0, "stream stride too small"),
    (2, ROW, FB, ROW, -FB, "stream stride too small"),
]
# One frame spans at most INT32_MAX bytes, (h - 1) * stride + w * channels (include/lvm_hip.h): the kernels address inside a frame with
# 32 bits.  SPAN_STRIDE is the largest row stride inside the bound for these frames; a refused call takes its arguments and touches no
# memory, so the rows just over it need no large buffer.  (Just inside: test_layout_emu_frame_span_just_inside_the_bound_is_accepted.)
SPAN_MSG = "frame rows span more than 2 GiB"
SPAN_STRIDE = (2**31 - 1 - ROW) // (H - 1)
assert (H - 1) * SPAN_STRIDE + ROW <= 2**31 - 1 < (H - 1) * (SPAN_STRIDE + 1) + ROW
REFUSED += [
    (1, SPAN_STRIDE + 1, FB, ROW, FB, SPAN_MSG),
    (1, ROW, FB, SPAN_STRIDE + 1, FB, SPAN_MSG),
    (2, SPAN_STRIDE + 1, FB, ROW, FB, SPAN_MSG),
    (2, ROW, FB, SPAN_STRIDE + 1, FB, SPAN_MSG),
    (1, 2**32 + ROW, FB, ROW, FB, SPAN_MSG),          # a stride whose low 32 bits are a legal one
    (1, ROW, FB, 2**32 + ROW, FB, SPAN_MSG),
    (1, 2**62, FB, ROW, FB, SPAN_MSG),                # (h - 1) * stride itself overflows 64 bits
]


def _launches(ctx):
    return sum(n for (_, n) in ctx.profile_collect().values())


@pytest.mark.parametrize("ns,si,ssi,so,sso,msg", REFUSED, ids=_ids([r[:5] for r in REFUSED]))
@pytest.mark.parametrize("api", ["device", "frames_first", "frames_batch"])
def test_layout_emu_bad_strides_are_refused_and_the_clip_continues(lvm, po, emu, ns, si, ssi, so, sso, msg, api):
    """A refused call launches nothing, writes nothing and leaves the state alone: the frames around it equal the oracle's bit for
    bit, as a clip without the refused calls.  `frames_first`: a batch call whose first frame goes through the per-frame path;
    `frames_batch`: one in steady state, where the frames would share launches."""
    ck, pk = lvm.synth.config(0, (W, H, LEVELS))
    clips = [lvm.synth.Clip(seed=1234 + s, **ck) for s in range(ns)]
    P, cp = po.make_params(**pk), c_params(lvm, pk)
    ctx = lvm.Context(0, ns, emu)
    ctx.exact_lab(True)
    ctx.profile(True)
    orcs = [po.Oracle() for _ in range(ns)]
    frames = np.stack([np.stack([c.frame(t) for c in clips]) for t in range(8)])         # [frame][stream][h][w][3]
    d_in = HOST.upload(frames)
    d_out = HOST.upload(np.full_like(frames, 0xCD))

    def good(t, nf):
        prod = ctx.process_device_frames(cp, nf, HOST.ptr(d_in, t), W, H, 3, ROW, FB, FB * ns, HOST.ptr(d_out, t), ROW, FB, FB * ns)
        ctx.synchronize()
        for f in range(t, t + nf):
            for s in range(ns):
                ref, pr = orcs[s].process(frames[f, s], P)
                assert pr == prod[f - t]
                assert np.array_equal(d_out[f, s], ref), "frame %d stream %d" % (f, s)

    def bad(t):
        before, launched = d_out.copy(), _launches(ctx)
        with pytest.raises(lvm.LvmError, match=msg):
            if api == "device":
                ctx.process_device(cp, HOST.ptr(d_in, t), W, H, 3, si, ssi, HOST.ptr(d_out, t), so, sso)
            else:
                ctx.process_device_frames(cp, 3, HOST.ptr(d_in, t), W, H, 3, si, ssi, FB * ns, HOST.ptr(d_out, t), so, sso, FB * ns)
        ctx.synchronize()
        assert _launches(ctx) == launched, "a refused call launched kernels"
        assert np.array_equal(d_out, before), "a refused call wrote to the output"
    try:
        if api == "frames_first":
            bad(0)                          # before any state exists
        good(0, 1)
        good(1, 3)
        bad(4)                              # steady state: device -> per-frame path, frames_* -> the batch leg must not take it
        good(4, 4)
    finally:
        ctx.close()
        for o in orcs:
            o.close()


@pytest.mark.parametrize("side", ["in", "out"])
def test_layout_emu_frame_span_just_inside_the_bound_is_accepted(lvm, po, emu, side):
    """The largest row stride of the bound, SPAN_STRIDE, on real memory: one allocation of 2 GiB whose pages are committed only where a
    row lies (np.empty), the other side packed.  Three Laplace frames equal the oracle's bit for bit; on the output side the 64 bytes
    behind every row stay 0xCD."""
    from numpy.lib.stride_tricks import as_strided
    ck, pk = lvm.synth.config(0, (W, H, LEVELS))
    clip = lvm.synth.Clip(**ck)
    P, cp = po.make_params(**pk), c_params(lvm, pk)
    guard = 64
    far = np.empty((H - 1) * SPAN_STRIDE + ROW + guard, np.uint8)
    rows = as_strided(far, shape=(H, ROW + guard), strides=(SPAN_STRIDE, 1))
    packed = np.zeros((H, ROW), np.uint8)
    ctx = lvm.Context(0, 1, emu)
    ctx.exact_lab(True)
    orc = po.Oracle()
    try:
        for t in range(3):
            f = clip.frame(t)
            ref, pr = orc.process(f, P)
            if side == "in":
                rows[:, :ROW] = f.reshape(H, ROW)
                rows[:, ROW:] = 0xAB
                packed[...] = 0xCD
                pg = ctx.process_device(cp, far.ctypes.data, W, H, 3, SPAN_STRIDE, far.size, packed.ctypes.data, ROW, FB)
            else:
                packed[...] = f.reshape(H, ROW)
                rows[...] = 0xCD
                pg = ctx.process_device(cp, packed.ctypes.data, W, H, 3, ROW, FB, far.ctypes.data, SPAN_STRIDE, far.size)
            ctx.synchronize()
            assert pg == pr and pr
            got = packed if side == "in" else rows[:, :ROW]
            assert np.array_equal(got.reshape(H, W, 3), ref), "frame %d: %d bytes differ" % (t, int((got.reshape(H, W, 3) != ref).sum()))
            if side == "out":
                assert (rows[:, ROW:] == 0xCD).all(), "frame %d: bytes behind the rows were written" % t
    finally:
        ctx.close()
        orc.close()
        del rows, far


def test_layout_emu_refused_batch_call_reserves_no_float_frame(lvm, emu):
    """lvm_debug_keep_float: the batch entry point sizes the kept float frame up front -- not for a layout it is about to refuse"""
    ck, pk = lvm.synth.config(0, (W, H, LEVELS))
    ctx = lvm.Context(0, 1, emu)
    ctx.keep_float(True)
    buf = HOST.upload(np.zeros((2, 3, H, W, 3), np.uint8))
    try:
        with pytest.raises(lvm.LvmError, match="frame stride too small"):
            ctx.process_device_frames(c_params(lvm, pk), 3, HOST.ptr(buf, 0), W, H, 3, ROW - 1, FB, FB, HOST.ptr(buf, 1), ROW, FB, FB)
        with pytest.raises(lvm.LvmError, match="no float frame kept"):
            ctx.read_float((H, W, 3))
    finally:
        ctx.close()


def test_layout_emu_mosaic_stream_stride_is_legal(lvm, po, emu):
    """the other side of the rule: a stream stride smaller than a frame (LAYOUTS F) is not refused"""
    M.layout_case(lvm, po, emu, HOST, 0, 64, 48, 3, 2, "F_device")


# ---- gfx950 build ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    return TorchMem()


@pytest.mark.gpu
@pytest.mark.parametrize("idx,w,h,levels,ns,name", M.LAYOUT_CASES, ids=_ids(M.LAYOUT_CASES))
def test_layout_gpu(lvm, po, hip, dev, idx, w, h, levels, ns, name):
    """Laplace, Color: bit for bit.  Riesz: the bars against the oracle and the bytes of the packed layout."""
    worst, _ = M.layout_case(lvm, po, hip, dev, idx, w, h, levels, ns, name, exact=idx != 2)
    if idx == 2:
        print("riesz layout", name, (w, h, levels), "streams", ns, "vs oracle: worst u8 diff %d, worst identical fraction %.6f" % tuple(worst))


@pytest.mark.gpu
@pytest.mark.parametrize("force,name", M.LAYOUT_FORCED_CASES, ids=_ids(M.LAYOUT_FORCED_CASES))
def test_layout_gpu_forced_strip_kernels(lvm, po, hip, dev, force, name):
    idx = M.LAYOUT_FORCED[force][0]
    worst, launched = M.layout_forced_case(lvm, po, hip, dev, force, name, exact=idx != 2)
    print("forced", force, "layout", name, "launched as asserted:", launched)
    if idx == 2:
        print("riesz forced layout", name, "vs oracle: worst u8 diff %d, worst identical fraction %.6f" % tuple(worst))
