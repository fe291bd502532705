"""Schedule equivalence on the gfx950 build, byte for byte, in the shipped configuration (no keep_float, default flavour).

include/lvm_hip.h promises that lvm_process_device_frames IS n_frames calls of lvm_process_device in order, and that pipeline
depth 1 gives results identical to depth 0.  The parity tests compare each schedule with the oracle only at the parity bars (1 LSB,
99.9 % identical), which a schedule that moved 0.1 % of the pixels by one level would pass.  Here one clip goes through every
surface (helpers.run_schedules) and every produced frame must carry the same bytes; one schedule is compared with the oracle.

Shapes: the BASELINE 1080p geometries, where the kernel choice flips with the launch size (Riesz: wave-strip collapse in batches,
tiled k_rz_final per frame; the output strip heights of Laplace and Color shrink with the task count), and an odd shape (byte
kernels).  All schedules use the same packed rows.  Not asserted: byte identity across memory layouts -- with a dword-aligned and
an odd row stride Laplace runs k_lap_final_v4 and k_lap_final, which associate the float sum differently (7 of 864 000 values,
1 LSB each, at 320 x 180 on the emulation build; both float frames within 5.7e-7 of the oracle's).

Also here: the two reference quirks of the framerate parameter on the GPU (Riesz keeps the framerate it was built with; Color
drops one window column per frame when the framerate falls)."""
import numpy as np
import pytest

from helpers import TorchMem, assert_schedules_identical, c_params, color_shrink_in_batches, oracle_bars, run_pair, run_schedules

pytestmark = pytest.mark.gpu

CALLS = (1, 7, 32, 5, 16)          # ragged temporal batches (61 frames): a seed frame, short, the bench's 32, odd, a power of two


def _clip(lvm, idx, size, fps=None):
    ck, pk = lvm.synth.config(idx, size)
    if fps is not None:
        ck["fps"] = fps; pk["framerate"] = fps
    clip = lvm.synth.Clip(**ck)
    other = lvm.synth.Clip(**dict(ck, seed=4321))
    n = sum(CALLS)
    return np.stack([clip.frame(t) for t in range(n)]), np.stack([other.frame(t) for t in range(n)]), pk


@pytest.mark.parametrize("idx,size,fps,n_oracle", [
    (1, None, None, 6),                 # Laplace 1920 x 1080, 6 levels
    (0, (323, 211, 5), None, 61),       # Laplace, odd shape (byte kernels)
    (2, None, None, 5),                 # Riesz 1920 x 1080, 6 levels: strips in batches, k_rz_final per frame
    (2, (323, 211, 5), None, 61),       # Riesz, odd shape (k_rz_final without vector I/O)
    (3, None, 15.0, 40),                # Color 1920 x 1080, 6 levels; fps 15: a 32-frame window, full inside the third call
    (3, (323, 211, 4), 15.0, 61),       # Color, odd shape
])
def test_schedules_give_identical_bytes(lvm, po, hip, idx, size, fps, n_oracle):
    frames, other, pk = _clip(lvm, idx, size, fps)
    res = run_schedules(lvm, hip, TorchMem(), frames, other, pk, CALLS, pipeline=(pk["mode"] == 0))
    assert_schedules_identical(res)
    prod, outs = res["frames_max"]
    worst = oracle_bars(po, frames, pk, prod, outs, n_oracle)
    print("mode", pk["mode"], frames.shape[1:3], "schedules", sorted(res), "oracle worst u8 / identical", worst)


def test_riesz_keeps_the_framerate_it_was_built_with(lvm, po, hip):
    """TemporalFilter.cpp:299-327: the Butterworth coefficients are computed from the framerate of the first frame; a later framerate
    change alone rebuilds nothing, and a coLow change rebuilds them with the OLD framerate.  Oracle and library at the bars, and the
    library's bytes equal a run whose framerate never changed."""
    ck, pk = lvm.synth.config(2, (320, 180, 4))

    def vary(t, p, fr=15.0):
        if t >= 4:
            p["framerate"] = fr
        if t >= 7:
            p["coLow"] = 1.0
        return p
    worst = run_pair(lvm, po, hip, lvm.synth.Clip(**ck), pk, 12, 1e-4, param_fn=vary)
    print("riesz framerate change worst", worst)
    clip = lvm.synth.Clip(**ck)
    outs = []
    for fr in (15.0, pk["framerate"]):
        ctx = lvm.Context(0, 1, hip)
        try:
            got = []
            for t in range(12):
                o, p = ctx.process(clip.frame(t), c_params(lvm, vary(t, dict(pk), fr)))
                got.append((p, np.array(o, copy=True)))
        finally:
            ctx.close()
        outs.append(got)
    for t, ((pa, a), (pb, b)) in enumerate(zip(*outs)):
        assert pa == pb and np.array_equal(a, b), "frame %d: the framerate change changed the output" % t


def test_color_window_shrinks_in_temporal_batches(lvm, po, hip):
    """framerate 60 -> 7 at frame 40 (window cap 128 -> 16: 24 frames of shrinking), calls 5, 16, 13 across the shrink"""
    worst = color_shrink_in_batches(lvm, po, hip, TorchMem(), (320, 180, 4), (1, 7, 32, 5, 16, 13), 40, 7.0, 1, 0.999)
    print("color shrink worst u8 / identical", worst)
