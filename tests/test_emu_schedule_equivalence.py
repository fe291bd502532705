"""CPU twin of tests/test_gpu_schedule_equivalence.py on the emulation build: at small shapes one clip through every surface of the
library in the shipped configuration (no keep_float, default flavour), identical produced flags and bytes in every schedule; and the
two framerate quirks of the reference bit-exact against the oracle."""
import numpy as np
import pytest

from helpers import HostMem, assert_schedules_identical, c_params, color_shrink_in_batches, oracle_bars, run_pair, run_schedules

CALLS = (1, 7, 12, 5, 4)           # ragged temporal batches (29 frames)


@pytest.mark.parametrize("idx,size,fps", [(0, (160, 90, 4), None), (0, (67, 45, 3), None), (2, (128, 72, 3), None), (2, (67, 45, 3), None),
                                          (3, (64, 48, 2), 7.0), (3, (67, 45, 2), 7.0)])    # Color at 7 fps: a 16-frame window, full in the third call
def test_emu_schedules_give_identical_bytes(lvm, po, emu, idx, size, fps):
    ck, pk = lvm.synth.config(idx, size)
    if fps is not None:
        ck["fps"] = fps; pk["framerate"] = fps
    n = sum(CALLS)
    clip, other = lvm.synth.Clip(**ck), lvm.synth.Clip(**dict(ck, seed=4321))
    frames = np.stack([clip.frame(t) for t in range(n)])
    res = run_schedules(lvm, emu, HostMem(), frames, np.stack([other.frame(t) for t in range(n)]), pk, CALLS, pipeline=(pk["mode"] == 0))
    assert_schedules_identical(res)
    prod, outs = res["frames"]
    oracle_bars(po, frames, pk, prod, outs, n)


def test_emu_riesz_keeps_the_framerate_it_was_built_with(lvm, po, emu):
    """TemporalFilter.cpp:299-327: a framerate change alone rebuilds nothing, a later coLow change rebuilds the Butterworth
    coefficients with the framerate of the first frame.  Bit-exact against the oracle, and for both oracle and library the bytes
    equal a run whose framerate never changed."""
    ck, pk = lvm.synth.config(2, (96, 64, 3))

    def vary(t, p, fr=15.0):
        if t >= 4:
            p["framerate"] = fr
        if t >= 7:
            p["coLow"] = 1.0
        return p
    run_pair(lvm, po, emu, lvm.synth.Clip(**ck), pk, 12, 0.0, exact=True, param_fn=vary)
    clip = lvm.synth.Clip(**ck)
    runs = []
    for fr in (15.0, pk["framerate"]):
        ctx, orc = lvm.Context(0, 1, emu), po.Oracle()
        try:
            got = []
            for t in range(12):
                p = vary(t, dict(pk), fr)
                o, pr = ctx.process(clip.frame(t), c_params(lvm, p))
                ref, pref = orc.process(clip.frame(t), po.make_params(**p))
                got.append((pr, np.array(o, copy=True), pref, np.array(ref, copy=True)))
        finally:
            ctx.close(); orc.close()
        runs.append(got)
    for t, (a, b) in enumerate(zip(*runs)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]), "frame %d: the framerate change changed the library's output" % t
        assert a[2] == b[2] and np.array_equal(a[3], b[3]), "frame %d: the framerate change changed the oracle's output" % t


def test_emu_color_window_shrinks_in_temporal_batches(lvm, po, emu):
    """framerate 60 -> 7 at frame 24 (window cap 128 -> 16: 8 frames of shrinking), calls of 3, 4 and 6 frames across the shrink;
    Color has no Lab arithmetic, so the shipped flavour is bit-exact"""
    color_shrink_in_batches(lvm, po, emu, HostMem(), (64, 48, 2), (1, 7, 16, 3, 4, 6), 24, 7.0, 0, 1.0)
